// host_predict.inc — candidate sets, prediction (fused / step-by-step / resident-inverse paths), gradients w.r.t.
// candidates, covariances (included by bosship.hip).

// ------------------------------------------------------------------------------------------
// candidates + prediction
// ------------------------------------------------------------------------------------------
extern "C" int boss_cand_create(int device, int d, int M, const double* Xs, boss_cand_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || M < 1 || !Xs) return fail(BOSS_E_INVALID, "need d >= 1, M >= 1 and non-NULL Xs");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    boss_cand* cd = new boss_cand();
    cd->ctx = c;
    cd->d = d;
    cd->M = M;
    cd->Mp = round_up(M, 64);
    if (dev_malloc((void**)&cd->Craw, sizeof(double) * d * cd->Mp) != hipSuccess) {
        delete cd;
        return fail(BOSS_E_ALLOC, "device allocation failed");
    }
    std::vector<double> buf;
    pack_points(buf, Xs, d, M, cd->Mp, nullptr);
    HIPCHK(hipMemcpy(cd->Craw, buf.data(), sizeof(double) * d * cd->Mp, hipMemcpyHostToDevice));
    *out = cd;
    return BOSS_OK;
}

// One-shot entry points (predict / predict_cov / predict_grad / acq_ei_grad) share one staging and one finish:
//  - candidates go into a grow-only per-device workspace instead of an allocation (hipMalloc/hipFree synchronise the device and
//    cost a few hundred microseconds per call): temp_cand, or ngp_pack + ngp_upload for the nonstationary calls;
//  - the outputs lie first and together in the c->pred workspace, inputs (prior means) behind them, and finish() copies them back;
//  - an error that follows enqueued work synchronises the stream before the call returns (drain), and the call frees what it
//    allocated: the next call reuses the workspaces right away.
// Caller holds the context lock.
static int drain(Ctx* c, int rc) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

// the error _clip_var raises (gaussian_process.jl:165,182): bad is the first offending candidate, v its variance
static int neg_var_error(long* bad_index, unsigned long long bad, double v) {
    if (bad_index) *bad_index = (long)bad;
    char msg[160];
    std::snprintf(msg, sizeof msg, "The posterior GP predicted variance %g but only values above -1e-08 are tolerated. (DomainError)", v);
    return fail(BOSS_E_NEG_VAR, msg);
}

struct DownCopy {
    void* host;
    const void* dev;
    size_t bytes;
};
// Copy the outputs back, synchronise, report a failed launch.  Outputs that lie together on the device and fit the pinned area come
// back in ONE copy (five copies into the caller's pageable arrays cost ≈60 µs of a ≈100 µs call), others one copy each.
static int finish(Ctx* c, std::initializer_list<DownCopy> outs) {
    hipStream_t s = c->stream;
    const char* next = (const char*)outs.begin()->dev;
    size_t total = 0;
    bool together = true;
    for (const DownCopy& o : outs) {
        together = together && o.dev == next;
        next = (const char*)o.dev + o.bytes;
        total += o.bytes;
    }
    hipError_t e;
    if (together && total <= PINNED_DOWN_BYTES) {
        char* stage = (char*)c->pinned + PINNED_DOWN_OFF;
        (void)hipMemcpyAsync(stage, outs.begin()->dev, total, hipMemcpyDeviceToHost, s);
        e = hipStreamSynchronize(s);
        for (const DownCopy& o : outs) {
            std::memcpy(o.host, stage, o.bytes);
            stage += o.bytes;
        }
    } else {
        for (const DownCopy& o : outs) (void)hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, s);
        e = hipStreamSynchronize(s);
    }
    const hipError_t e2 = hipGetLastError();                 // (read either way: it also clears the error)
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    return BOSS_OK;
}

static int temp_cand(Ctx* c, int d, int M, const double* Xs, boss_cand* cd) {
    cd->ctx = c;
    cd->d = d;
    cd->M = M;
    cd->Mp = round_up(M, 64);
    int rc = ws_reserve(c->craw, sizeof(double) * (size_t)d * cd->Mp);
    if (rc) return rc;
    cd->Craw = (double*)c->craw.p;
    std::vector<double> buf;
    pack_points(buf, Xs, d, M, cd->Mp, nullptr);
    const size_t bytes = sizeof(double) * d * cd->Mp;
    if (bytes <= PINNED_UP_BYTES) {
        // few candidates: stage through pinned memory, no synchronisation (every entry point that calls this ends with
        // a stream synchronisation before it returns, so the area is free again at the next call)
        void* stage = (char*)c->pinned + PINNED_UP_OFF;
        HIPCHK(hipEventSynchronize(c->ev_up));             // the previous upload from this area (normally long complete)
        std::memcpy(stage, buf.data(), bytes);
        HIPCHK(hipMemcpyAsync(cd->Craw, stage, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->ev_up, c->stream));
        return BOSS_OK;
    }
    HIPCHK(hipMemcpyAsync(cd->Craw, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));               // staging buffer goes out of scope
    return BOSS_OK;
}

extern "C" void boss_cand_free(boss_cand_t* cd) {
    if (!cd) return;
    if (cd->ctx) {
        (void)hipSetDevice(cd->ctx->device);
        (void)hipStreamSynchronize(cd->ctx->stream);
    }
    if (cd->Craw) (void)hipFree(cd->Craw);
    delete cd;
}

// scaled (and, for DiscreteKernel dims, rounded) candidates for one GP
__global__ void scale_cand_kernel(const double* __restrict__ Craw, double* __restrict__ Csc, const double* __restrict__ invlam,
                                  const unsigned char* __restrict__ discrete, int d, int Mp) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Mp) return;
    for (int k = 0; k < d; ++k) {
        double v = Craw[(size_t)k * Mp + j];
        if (discrete && discrete[k]) v = rint(v);
        Csc[(size_t)k * Mp + j] = v * invlam[k];
    }
}

// candidate tiles (of 32) up to which the resident-inverse GEMMs replace the step-by-step substitution (measured at N=4096:
// 0.19 vs 0.59 ms at 7 tiles, 0.46 vs 0.85 ms at 32, 0.75 vs 1.16 ms at 64, 1.36 vs 1.85 ms at 128 = the whole few-candidates range)
static int invgemm_max_tiles() {
    static const int v = getenv("BOSS_INVGEMM_MAX_TILES") ? atoi(getenv("BOSS_INVGEMM_MAX_TILES")) : 128;
    return v;
}
// the few-candidates paths (prediction, its gradient, the arg-max rounds of host_prune.inc): BOSS_NO_FEW=1 switches them off,
// BOSS_FEW_MAX_TILES is the number of candidate tiles (of 32) up to which they are taken
static bool few_off() {
    static const bool v = getenv("BOSS_NO_FEW") && atoi(getenv("BOSS_NO_FEW"));
    return v;
}
static int few_max_tiles() {
    static const int v = getenv("BOSS_FEW_MAX_TILES") ? atoi(getenv("BOSS_FEW_MAX_TILES")) : 128;
    return v;
}
// BOSS_NO_SET_PREDICT=1: calls over several posteriors go member by member, never through the set launches
static bool set_predict_off() {
    static const bool v = getenv("BOSS_NO_SET_PREDICT") && atoi(getenv("BOSS_NO_SET_PREDICT"));
    return v;
}

// width of the V slabs predict_enqueue leaves (and the covariances read): 64 candidates per workgroup once that still fills the
// machine (BOSS_FORCE_BN64=1: tests); the gradient pass (adjoint substitution) runs on 32-candidate slabs
static int slab_bn(int M, bool for_grad) {
    static const bool force64 = getenv("BOSS_FORCE_BN64") && atoi(getenv("BOSS_FORCE_BN64"));
    return !for_grad && (M >= 64 * 256 || force64) ? 64 : 32;
}


// U = L⁻ᵀ (upper, leading dimension g->ld) by recursive doubling from the 256×256 diagonal inverses; Lw (same shape)
// is the lower work matrix.  Dinv2 must be current on stream s.
static void linv_enqueue(boss_gp* g, hipStream_t s, double* U, double* Lw, const SetBatch& B) {
    const int Np = g->Np, ld = g->ld;
    hipLaunchKernelGGL(linv_seed_kernel, dim3(PRED_RB, Np / PRED_RB, B.nb), dim3(PRED_RB), 0, s, (const double*)g->Dinv2, Lw, ld, U, ld,
                       B.sDinv2, B.sW);
    for (int sz = PRED_RB; sz < Np; sz *= 2) {
        const int pairs = (Np + 2 * sz - 1) / (2 * sz), tiles = (sz / BLK) * (sz / BLK);
        hipLaunchKernelGGL((linv_level_kernel<SyrkG, 1>), dim3(tiles, pairs, B.nb), dim3(256), 0, s, (const double*)g->A, ld, Lw, ld, U, ld,
                           Np, sz, B.sA, B.sW);
        hipLaunchKernelGGL((linv_level_kernel<SyrkG, 2>), dim3(tiles, pairs, B.nb), dim3(256), 0, s, (const double*)g->A, ld, Lw, ld, U, ld,
                           Np, sz, B.sA, B.sW);
    }
}

// Gibbs-kernel cross-covariances into 32-wide tiles: lanes along the candidate columns while the staging fits in LDS
static void gibbs_kstar32_launch(boss_gp* g, const boss_cand* cd, const double* clam_dev, const double* camp_dev, int tiles,
                                 double* out, hipStream_t s) {
    if (g->d <= GIBBS_KSTAR_MAX_D)
        hipLaunchKernelGGL(gibbs_kstar_cols_kernel, dim3(g->Np / 256, tiles), dim3(256),
                           sizeof(double) * (2 * g->d * 32 + 32 + 2 * 8 * 256), s, (const double*)g->Xraw, (const double*)g->lamX,
                           (const double*)g->ampX, g->d, g->N, g->Np, (const double*)cd->Craw, clam_dev, camp_dev, cd->Mp, out);
    else
        hipLaunchKernelGGL(gibbs_kstar_kernel<32>, dim3(g->Np / 256, tiles), dim3(256), sizeof(double) * (2 * g->d + 1) * 32, s,
                           (const double*)g->Xraw, (const double*)g->lamX, (const double*)g->ampX, g->d, g->N, g->Np,
                           (const double*)cd->Craw, clam_dev, camp_dev, cd->Mp, out);
}

// enqueue μ/σ² (unclipped) of one posterior at resident candidates into device arrays mu, var (length ≥ M)
// L⁻¹ of a posterior with N <= 128 = block 0 of the block inverses: one 8-wave launch instead of the four of dinv_launch
static void small_dinv(boss_gp* g, hipStream_t s) {
    dinv_join(g);
    if (g->have_dinv || g->dinv0_gen == g->factor_gen) return;
    hipLaunchKernelGGL(potrf_dinv_kernel, dim3(8, 1, 1), dim3(64), 0, s, g->A, g->ld, (size_t)0, g->inv16, (size_t)0, g->Dinv, (size_t)0);
    g->dinv0_gen = g->factor_gen;
}
static bool small_predict_ok(const boss_gp* g, int M) {
    // one wave per candidate costs ∝ N² per candidate: up to 1024 candidates at N = 128, proportionally more below (the tiled
    // kernels take over where they are faster: 251 against 367 µs at N = 100, M = 8192)
    const long long cap = std::min<long long>(16384, 1024LL * SMALL_MAX_N * SMALL_MAX_N / ((long long)g->N * g->N));
    return small_fit_ok(g->ctx, g->N, g->d) && M <= cap && !g->aug && !g->gibbs && !g->kprog;
}

static int predict_enqueue(boss_gp* g, const boss_cand* cd, const double* mean_s_dev, double* mu, double* var,
                           bool for_grad = false, const double* clam_dev = nullptr, const double* camp_dev = nullptr,
                           bool need_v = false, bool internal = false) {
    // need_v: the caller reads V = L⁻¹K* from the slab scratch afterwards (covariances); for_grad implies it
    // internal: a round of the arg-max-only acquisition (host_prune.inc) — it does not count as a few-candidates call of the user's
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    if (g->gibbs && !clam_dev)
        return fail(BOSS_E_INVALID, "nonstationary posteriors predict through boss_ngp_predict (λ(x*), α(x*) are needed)");
    // (for_grad also keeps the 32-wide V slabs for a new track: the gradient entry points check boss_kgp_set_grad themselves, the
    // track's asks for boss_kgp_set_sequential)
    if (g->kprog && ((for_grad && !g->kgrad && !g->kseq) || need_v))
        return fail(BOSS_E_INVALID, "not available for program-kernel posteriors (boss_kgp_create): covariances, and gradients without boss_kgp_set_grad");
    if (cd->ctx != c) return fail(BOSS_E_INVALID, "candidates and posterior live on different devices");
    if (cd->d != g->d) return fail(BOSS_E_INVALID, "candidate dimension differs from the model's x_dim");
    if (!for_grad && !need_v && small_predict_ok(g, cd->M)) {
        // N <= 128, few enough candidates (small_predict_ok): scaling, K*, substitution and moments in ONE launch against L⁻¹ in LDS
        small_dinv(g, s);
        const int grid = std::min(512, (cd->M + SPG_WAVES - 1) / SPG_WAVES);
        hipLaunchKernelGGL(small_predict_grad_kernel<false>, dim3(grid), dim3(SPG_THREADS), SPG_LDS_BYTES, s, (const double*)g->Dinv,
                           (const double*)g->A, g->ld, g->Np, g->N, g->d, g->kernel, g->amp2, (const double*)g->Xsc, g->ldx,
                           (const double*)cd->Craw, cd->Mp, cd->M, (const double*)g->invlam, (const unsigned char*)g->discrete_dev,
                           mean_s_dev, (const double*)nullptr, mu, var, (double*)nullptr, (double*)nullptr);
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    }
    // The block inverses may still be in the making on the side stream (dinv_eager): the main stream joins it where the first kernel
    // that reads them is enqueued — candidate scaling and K* of the few-candidates path run beside their tail.
    bool joined = false;
    auto join_dinv = [&]() {
        if (!joined) dinv_join(g);
        joined = true;
    };
    if (!g->have_dinv) {
        join_dinv();
        ProfScope ps(c, "dinv");
        dinv_launch(g, s);
        g->have_dinv = true;
    }
    g->dinv_used = true;
    const int Mp = cd->Mp;
    const int BN = slab_bn(cd->M, for_grad);
    const int tiles = (cd->M + BN - 1) / BN;
    int rc = ws_reserve(c->csc, sizeof(double) * (size_t)g->d * Mp);
    if (rc) return rc;
    rc = ws_reserve(c->vscratch, sizeof(double) * (size_t)tiles * BN * g->Np * (for_grad ? 2 : 1));   // gradients: V and W slabs
    if (rc) return rc;
    double* Csc = (double*)c->csc.p;
    double* kpv = nullptr;                                   // program kernel: k(x*, x*) per candidate, written beside K*
    if (g->kprog) {
        rc = ws_reserve(c->kpv, sizeof(double) * (size_t)Mp);
        if (rc) return rc;
        kpv = (double*)c->kpv.p;
    }
    const int vmode = g->aug ? 1 : (g->gibbs || g->kprog) ? 2 : 0;   // how the finish kernels leave σ² (predict_kernels.hpp)
    if (!g->gibbs)
        hipLaunchKernelGGL(scale_cand_kernel, dim3((Mp + 255) / 256), dim3(256), 0, s, cd->Craw, Csc, g->invlam,
                           g->discrete_dev, g->d, Mp);
#ifdef BOSS_EXPERIMENTS
    static const int dbg = getenv("BOSS_DBG") ? atoi(getenv("BOSS_DBG")) : 0;   // work-skipping switches: experiment builds only
#else
    constexpr int dbg = 0;
#endif
    const int ftiles = (cd->M + 31) / 32;
    const size_t aug_lds = sizeof(double) * ((size_t)g->d * (64 + 256) + g->d);
    if (ftiles <= few_max_tiles() && g->Np >= 4 * PRED_RB && g->d <= 64 && !few_off() && (BN == 32 || for_grad)) {
        // few candidates (the fused kernel would occupy `ftiles` of 256 CUs for its whole latency):
        // right-looking substitution, every 256-row step spread over the chip
        typedef PredG32 G;
        typedef GemmDirect<4, 1, 2, 2, 8> GU;                // 128×32 update tiles
        ProfScope ps(c, "predict");
        const int nb = g->Np / PRED_RB;
        const int nwg = g->Np / WINV_ROWS;
        const size_t step_part = (size_t)ftiles * nb * FEW_STEP_PARTS * 64;     // per-step partial sums of the one-launch-per-step form
        rc = ws_reserve(c->few, sizeof(double) * ((size_t)ftiles * ((size_t)g->Np * 32 + 64) + (size_t)nwg * 8 + step_part));
        if (rc) return rc;
        double* R = (double*)c->few.p;                       // residuals [tile][Np][32], start as K*
        double* ssmz = R + (size_t)ftiles * g->Np * 32;
        double* part = ssmz + 64 * (size_t)ftiles + (size_t)nwg * 8;
        double* V = (double*)c->vscratch.p;
        // repeated calls with few candidates on one factorisation: from the second call on both inverse factors are
        // resident — one to four candidates take a single pass over L⁻ᵀ (winv_gemv_kernel), more take two GEMMs
        // without sequential steps (inv_fwd_kernel / inv_bwd_kernel)
        const size_t winv_lds = sizeof(double) * (size_t)g->Np * (cd->M == 1 ? 1 : cd->M == 2 ? 2 : WINV_MAX_M);   // K* staged in LDS
        if (winv_after() > 0 && !g->have_winv && !internal && ++g->few_calls >= winv_after()) {
            const size_t bytes = sizeof(double) * (size_t)g->ld * g->Np;
            bool ok = (g->Winv != nullptr || dev_malloc((void**)&g->Winv, bytes) == hipSuccess) &&
                      (g->Linv != nullptr || dev_malloc((void**)&g->Linv, bytes) == hipSuccess);
            if (ok) {
                join_dinv();
                linv_enqueue(g, s, g->Winv, g->Linv);
                g->have_winv = true;
            } else {
                (void)hipGetLastError();                 // no memory for the inverses: stay on the substitution path
                g->few_calls = -(1 << 30);
            }
        }
        const bool use_winv = g->have_winv && !for_grad && !need_v && cd->M <= WINV_MAX_M && winv_lds <= 144 * 1024;
        const bool use_invgemm = g->have_winv && !use_winv && ftiles <= invgemm_max_tiles();   // beyond: the step path is faster
        if (!use_winv) (void)hipMemsetAsync(ssmz, 0, sizeof(double) * 64 * ftiles, s);
        if (g->aug)
            hipLaunchKernelGGL(aug_kstar_kernel, dim3(g->Np / 256, ftiles), dim3(256), aug_lds, s, (const double*)g->Xraw, g->ldx,
                               g->d, g->nhead, g->N, g->Np, (const double*)cd->Craw, Mp, g->kernel, g->amp2,
                               (const double*)g->invlam, R, 32);
        else if (g->gibbs)
            gibbs_kstar32_launch(g, cd, clam_dev, camp_dev, ftiles, R, s);
        else if (g->kprog)
            kprog_kstar_launch(g, cd, Csc, 32, ftiles, R, kpv, s);
        else
            hipLaunchKernelGGL(kstar_rows_kernel, dim3(g->Np / 256, ftiles), dim3(256), sizeof(double) * (g->d * 32 + KSTAR_LDS_EXTRA), s,
                               (const double*)g->Xsc, g->Np, g->N, (const double*)Csc, g->d, Mp, g->kernel, g->amp2, R,
                               use_winv ? cd->M : 32);
        join_dinv();
        if (use_invgemm) {
            const int nrb = g->Np / BLK;
            rc = ws_reserve(c->lgC, sizeof(double) * (size_t)ftiles * nrb * 64);
            if (rc) return rc;
            double* ssp = (double*)c->lgC.p;
            hipLaunchKernelGGL(inv_fwd_kernel<GU>, dim3(ftiles, nrb), dim3(GU::NTHREADS), 0, s, (const double*)g->Linv, g->ld, g->Np,
                               (const double*)g->A, g->ld, (const double*)R, V, ssp);
            hipLaunchKernelGGL(inv_fwd_finish_kernel, dim3(ftiles), dim3(256), 0, s, (const double*)ssp, nrb, mean_s_dev, cd->M,
                               g->amp2, vmode, mu, var);
            if (g->gibbs) hipLaunchKernelGGL(gibbs_var_kernel, dim3((cd->M + 255) / 256), dim3(256), 0, s, var, camp_dev, cd->M);
            if (g->kprog) kprog_var_launch(s, var, kpv, cd->M);
            HIPCHK(hipGetLastError());
            return BOSS_OK;
        }
        if (use_winv) {
            double* part = ssmz + 64 * (size_t)ftiles;
            const int mc = cd->M == 1 ? 1 : cd->M == 2 ? 2 : 4;
            const size_t lds = sizeof(double) * (size_t)g->Np * mc;
            auto kfn = mc == 1 ? winv_gemv_kernel<1> : mc == 2 ? winv_gemv_kernel<2> : winv_gemv_kernel<4>;
            hipLaunchKernelGGL(kfn, dim3(nwg), dim3(256), lds, s, (const double*)g->Winv, g->ld, g->Np,
                               (const double*)g->A, g->ld, (const double*)R, cd->M, part, (double*)nullptr);
            hipLaunchKernelGGL(winv_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nwg, cd->M, mean_s_dev, g->amp2,
                               vmode, mu, var);
            if (g->gibbs) hipLaunchKernelGGL(gibbs_var_kernel, dim3(1), dim3(256), 0, s, var, camp_dev, cd->M);
            if (g->kprog) kprog_var_launch(s, var, kpv, cd->M);
            HIPCHK(hipGetLastError());
            return BOSS_OK;
        }
        static const bool few_w_off = getenv("BOSS_NO_FEW_W") && atoi(getenv("BOSS_NO_FEW_W"));
        if (!few_w_off && g->W2 && g->w2_np != g->Np) {      // (the handle's storage grew)
            (void)hipStreamSynchronize(s);
            (void)hipFree(g->W2);
            g->W2 = nullptr;
        }
        if (!few_w_off && !g->W2) {
            if (dev_malloc((void**)&g->W2, sizeof(double) * (size_t)nb * FEW_W_SLAB) == hipSuccess) {
                g->w2_np = g->Np;
                g->w2_gen = ~0ull;
            } else {
                (void)hipGetLastError();                     // no memory for it: the two-launch steps below
                g->W2 = nullptr;
            }
        }
        if (!few_w_off && g->W2) {
            // one launch per step (few_step_kernel): V_ib and, beside it, the update V_{ib-1} owes the blocks below block ib
            g->w2_used = true;
            if (g->w2_gen != g->factor_gen) {
                hipLaunchKernelGGL(few_w_kernel<G>, dim3(PRED_RB / 32, 2 * nb), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, (const double*)g->A,
                                   g->ld, (const double*)g->Dinv2, g->W2);
                g->w2_gen = g->factor_gen;
            }
            for (int ib = 0; ib < nb; ++ib) {
                const int nblk = ib >= 2 && (ib & 1) == 0 ? (nb - 1 - ib) * (PRED_RB / GU::BM) : 0;   // the pair update rides on even steps
                const int per_x = (nblk >> 3) * ftiles + ((nblk & 7) * ftiles + 7) / 8;
                hipLaunchKernelGGL(few_step_kernel<GU>, dim3(ftiles * FEW_STEP_PARTS + 8 * per_x), dim3(256), 0, s, (const double*)g->A, g->ld,
                                   g->Np, nb, ib, ftiles, R, (const double*)g->Dinv2, (const double*)g->W2, V, part);
            }
            hipLaunchKernelGGL(few_sum_kernel, dim3(ftiles), dim3(256), 0, s, (const double*)part, nb, mean_s_dev, cd->M, g->amp2, mu, var,
                               vmode);
            if (g->gibbs) hipLaunchKernelGGL(gibbs_var_kernel, dim3((cd->M + 255) / 256), dim3(256), 0, s, var, camp_dev, cd->M);
            if (g->kprog) kprog_var_launch(s, var, kpv, cd->M);
            HIPCHK(hipGetLastError());
            return BOSS_OK;
        }
        for (int ib = 0; ib < nb; ++ib) {
            hipLaunchKernelGGL(few_finish_kernel<G>, dim3(ftiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, (const double*)g->A,
                               g->ld, g->Np, ib, (const double*)R, (const double*)g->Dinv2, V, ssmz, ib == nb - 1 ? 1 : 0,
                               mean_s_dev, cd->M, g->amp2, mu, var, vmode);
            const int nupd = (nb - 1 - ib) * (PRED_RB / BLK);
            if (nupd > 0)
                hipLaunchKernelGGL(few_update_kernel<GU>, dim3(ftiles, nupd), dim3(GU::NTHREADS), 0, s, (const double*)g->A, g->ld,
                                   g->Np, ib, (const double*)V, R);
        }
        if (g->gibbs) hipLaunchKernelGGL(gibbs_var_kernel, dim3((cd->M + 255) / 256), dim3(256), 0, s, var, camp_dev, cd->M);
        if (g->kprog) kprog_var_launch(s, var, kpv, cd->M);
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    }
    join_dinv();
    if (g->aug || g->gibbs || g->kprog) {
        ProfScope ps(c, "predict");
        double* V = (double*)c->vscratch.p;
        // a program kernel's epilogue is the nonstationary one: −Σv² from the kernel, k(x*, x*) added behind it (KERN_PROGRAM itself
        // never reaches a kernel that evaluates kappa_*)
        const int pre_kern = g->kprog ? KERN_GIBBS : g->kernel;
        if (g->aug)
            hipLaunchKernelGGL(aug_kstar_kernel, dim3(g->Np / 256, tiles), dim3(256), aug_lds, s, (const double*)g->Xraw, g->ldx, g->d,
                               g->nhead, g->N, g->Np, (const double*)cd->Craw, Mp, g->kernel, g->amp2, (const double*)g->invlam, V, BN);
        else if (g->kprog)
            kprog_kstar_launch(g, cd, Csc, BN, tiles, V, kpv, s);
        else if (BN == 32)
            gibbs_kstar32_launch(g, cd, clam_dev, camp_dev, tiles, V, s);
        else
            hipLaunchKernelGGL(gibbs_kstar_kernel<64>, dim3(g->Np / 256, tiles), dim3(256), sizeof(double) * (2 * g->d + 1) * 64, s,
                               (const double*)g->Xraw, (const double*)g->lamX, (const double*)g->ampX, g->d, g->N, g->Np,
                               (const double*)cd->Craw, clam_dev, camp_dev, Mp, V);
        if (BN == 32) {
            typedef PredG32 G;
            hipLaunchKernelGGL((predict_kernel<G, true>), dim3(tiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, g->A, g->ld, g->Np,
                               g->N, g->Dinv2, g->Xsc, Csc, g->d, Mp, pre_kern, g->amp2, V, mean_s_dev, cd->M, mu, var, dbg);
        } else {
            typedef PredG64 G;
            hipLaunchKernelGGL((predict_kernel<G, true>), dim3(tiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, g->A, g->ld, g->Np,
                               g->N, g->Dinv, g->Xsc, Csc, g->d, Mp, pre_kern, g->amp2, V, mean_s_dev, cd->M, mu, var, dbg);
        }
        if (g->gibbs) hipLaunchKernelGGL(gibbs_var_kernel, dim3((cd->M + 255) / 256), dim3(256), 0, s, var, camp_dev, cd->M);
        if (g->kprog) kprog_var_launch(s, var, kpv, cd->M);
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    }
    {
        ProfScope ps(c, "predict");
        if (BN == 32) {
            typedef PredG32 G;
            hipLaunchKernelGGL(predict_kernel<G>, dim3(tiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, g->A, g->ld, g->Np,
                               g->N, g->Dinv2, g->Xsc, Csc, g->d, Mp, g->kernel, g->amp2, (double*)c->vscratch.p, mean_s_dev, cd->M, mu, var, dbg);
        } else {
            typedef PredG64 G;
            hipLaunchKernelGGL(predict_kernel<G>, dim3(tiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, g->A, g->ld, g->Np,
                               g->N, g->Dinv, g->Xsc, Csc, g->d, Mp, g->kernel, g->amp2, (double*)c->vscratch.p, mean_s_dev, cd->M, mu, var, dbg);
        }
    }
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// A SET of equally shaped posteriors at the same candidates in one prediction launch (predict_kernel_set): the S hyper-parameter
// samples (× P outputs) of a Bayesian-inference model, src/posterior.jl:15-19 / expected_improvement.jl:87-90.
// ------------------------------------------------------------------------------------------
__global__ void scale_cand_set_kernel(const double* __restrict__ Craw, const PredSet* __restrict__ sets,
                                      const unsigned char* __restrict__ discrete, int d, int Mp) {
    const PredSet ps = sets[blockIdx.y];
    double* Csc = const_cast<double*>(ps.Csc);
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Mp) return;
    for (int k = 0; k < d; ++k) {
        double v = Craw[(size_t)k * Mp + j];
        if (discrete && discrete[k]) v = rint(v);
        Csc[(size_t)k * Mp + j] = v * ps.invlam[k];
    }
}

static int set_np_max() {
    static const int v = getenv("BOSS_SET_NP_MAX") ? atoi(getenv("BOSS_SET_NP_MAX")) : 2048;
    return v;
}
// may the n posteriors be predicted by one launch?  (models of one kind and shape on the candidates' device, fused 32-candidate
// kernel: plain stationary models; gradient-observation models of one point count — the members of boss_ggp_fit_batch calls on the
// outputs of a model —; where the caller brings the latent values at the candidates (with_latents, boss_ngp_predict_set),
// nonstationary models; and the members of boss_kgp_fit_batch calls — program-kernel models — whose programs are bytewise equal)
static bool predict_set_ok(int n, boss_gp_t* const* gps, const boss_cand* cd, bool with_latents = false) {
    if (n < 2) return false;
    const boss_gp* g0 = gps[0];
    if (!g0 || g0->Np > set_np_max() || g0->ctx->prof_on || g0->d > 64) return false;
    if (g0->gibbs && (!with_latents || g0->d > GIBBS_KSTAR_MAX_D)) return false;
    const bool model = g0->aug || g0->gibbs;                 // K* comes from the members' raw points: one layout for all
    for (int i = 0; i < n; ++i) {
        const boss_gp* g = gps[i];
        if (!g || g->aug != g0->aug || g->gibbs != g0->gibbs || !g->fitted || g->pending || g->ctx != cd->ctx || g->N != g0->N || g->Np != g0->Np ||
            g->ld != g0->ld || g->d != g0->d || g->d != cd->d || g->kernel != g0->kernel || g->discrete != g0->discrete)
            return false;
        // program kernels: members of fitted sets (boss_kgp_fit_batch) under ONE program (the set launch carries it in its arguments);
        // a list that mixes built-in and program handles, or two programs, goes member by member, and so do handles that stand alone
        // (boss_kgp_create, or a member that was detached)
        if (g->kprog != g0->kprog || (g->kprog && (!g->set || std::memcmp(g->kp, g0->kp, sizeof(FitProg)) != 0))) return false;
        if (model && (g->npts != g0->npts || g->ldx != g0->ldx || g->nhead != g0->nhead)) return false;
    }
    return true;
}
// The diagonal-block inverses of every member of a set, current on the stream: members of ONE batch-fitted set that still lack them
// get them in one set of launches (grid.z = member; their arrays are views into one slab with constant strides), anything else member
// by member.  Idempotent.
static void set_dinv_enqueue(int n, boss_gp_t* const* gps, hipStream_t s) {
    boss_gp* g0 = gps[0];
    bool uniform = n >= 2 && g0->set != nullptr;
    const ptrdiff_t sA = n >= 2 ? gps[1]->A - gps[0]->A : 0, sI = n >= 2 ? gps[1]->inv16 - gps[0]->inv16 : 0,
                    sD = n >= 2 ? gps[1]->Dinv - gps[0]->Dinv : 0, sD2 = n >= 2 ? gps[1]->Dinv2 - gps[0]->Dinv2 : 0;
    for (int i = 0; i < n && uniform; ++i) {
        const boss_gp* g = gps[i];
        uniform = g->set == g0->set && !g->have_dinv && !g->dinv_pending && g->A - g0->A == sA * i && g->inv16 - g0->inv16 == sI * i &&
                  g->Dinv - g0->Dinv == sD * i && g->Dinv2 - g0->Dinv2 == sD2 * i && sA > 0 && sI > 0 && sD > 0 && sD2 > 0;
    }
    if (uniform) {
        SetBatch B;
        B.nb = n;
        B.sA = (size_t)sA;
        B.sInv16 = (size_t)sI;
        B.sDinv = (size_t)sD;
        B.sDinv2 = (size_t)sD2;
        dinv_launch(gps[0], s, B);
        for (int i = 0; i < n; ++i) gps[i]->have_dinv = true;
    }
    for (int i = 0; i < n; ++i) {
        boss_gp* g = gps[i];
        dinv_join(g);
        if (!g->have_dinv) {
            dinv_launch(g, s);
            g->have_dinv = true;
        }
        g->dinv_used = true;
    }
}
// moments of posteriors gps[0..n-1] at resident candidates: mu/var of posterior i at mu_all + i·mstride (unclipped); mean_all (or
// null): prior means at the candidates in the same layout.  Caller holds the context lock and has checked predict_set_ok.
// Gradient-observation and nonstationary members: K* of every member goes into its V slabs first (aug_kstar_set_kernel /
// gibbs_kstar_set_kernel), the substitution takes it from there (predict_kernel_set<G, true>); clam_all / camp_all are the
// nonstationary members' latent values at the candidates, [n][d][Mp] and [n][Mp].
// after_group(i0, cnt), if given, is called behind the launches of every group of members: their V slabs (member i0 + k, tile t at
// slab k·tiles + t of the scratch) are overwritten by the next group, so whoever needs them enqueues its work there (grad_set_enqueue).
static int predict_set_enqueue(int n, boss_gp_t* const* gps, const boss_cand* cd, const double* mean_all, double* mu_all,
                               double* var_all, size_t mstride, const double* clam_all = nullptr, const double* camp_all = nullptr,
                               const std::function<int(int, int)>* after_group = nullptr) {
    boss_gp* g0 = gps[0];
    Ctx* c = g0->ctx;
    hipStream_t s = c->stream;
    typedef PredG32 G;
    const int Mp = cd->Mp, d = g0->d, Np = g0->Np;
    const int tiles = (cd->M + G::BN - 1) / G::BN;
    set_dinv_enqueue(n, gps, s);
    // the V slabs of the workgroups in flight: groups of posteriors per launch so that the scratch stays bounded
    static const size_t v_cap = (size_t)(getenv("BOSS_SET_V_GIB") ? atof(getenv("BOSS_SET_V_GIB")) : 8.0) * ((size_t)1 << 30);
    const size_t v_one = sizeof(double) * (size_t)tiles * G::BN * Np;
    int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, std::min<size_t>(v_cap / v_one, 65535)));
    int rc = ws_reserve(c->vscratch, v_one * group);
    while (rc == BOSS_E_ALLOC && group > 1) {                // a full or shared device: fewer posteriors per launch instead of failing the call
        group = (group + 1) / 2;
        rc = ws_reserve(c->vscratch, v_one * group);
    }
    if (rc) return rc;
    const bool pre = g0->aug || g0->gibbs || g0->kprog;
    const bool own_csc = !g0->aug && !g0->gibbs;             // (K* from the member's scaled points: the candidates scaled per member)
    if (own_csc) rc = ws_reserve(c->csc, sizeof(double) * (size_t)d * Mp * n);
    if (rc) return rc;
    double* kpv = nullptr;                                   // program kernel: k(x*, x*) per member and candidate, written beside K*
    if (g0->kprog) {
        rc = ws_reserve(c->kpv, sizeof(double) * (size_t)Mp * n);
        if (rc) return rc;
        kpv = (double*)c->kpv.p;
    }
    rc = ws_reserve(c->setdesc, sizeof(PredSet) * (size_t)n);
    if (rc) return rc;
    std::vector<PredSet> desc(n);
    for (int i = 0; i < n; ++i) {
        const boss_gp* g = gps[i];
        desc[i].A = g->A;
        desc[i].Dinv = g->Dinv2;
        desc[i].Xsc = g->Xsc;
        desc[i].Csc = own_csc ? (const double*)c->csc.p + (size_t)i * d * Mp : nullptr;
        desc[i].mean_s = mean_all ? mean_all + (size_t)i * mstride : nullptr;
        desc[i].invlam = g->invlam;
        desc[i].mu = mu_all + (size_t)i * mstride;
        desc[i].var = var_all + (size_t)i * mstride;
        desc[i].amp2 = g->amp2;
        desc[i].Xraw = own_csc ? nullptr : g->Xraw;
        if (g->gibbs) {
            desc[i].lamX = g->lamX;
            desc[i].ampX = g->ampX;
            desc[i].clam = clam_all + (size_t)i * d * Mp;
            desc[i].camp = camp_all + (size_t)i * Mp;
        }
    }
    const size_t bytes = sizeof(PredSet) * (size_t)n;
    if (bytes <= PINNED_UP_BYTES) {
        void* stage = (char*)c->pinned + PINNED_UP_OFF;
        HIPCHK(hipEventSynchronize(c->ev_up));
        std::memcpy(stage, desc.data(), bytes);
        HIPCHK(hipMemcpyAsync(c->setdesc.p, stage, bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(c->ev_up, s));
    } else {
        HIPCHK(hipMemcpyAsync(c->setdesc.p, desc.data(), bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    const PredSet* dsets = (const PredSet*)c->setdesc.p;
    if (own_csc)
        for (int i0 = 0; i0 < n; i0 += 65535)
            hipLaunchKernelGGL(scale_cand_set_kernel, dim3((Mp + 255) / 256, std::min(65535, n - i0)), dim3(256), 0, s, (const double*)cd->Craw,
                               dsets + i0, (const unsigned char*)g0->discrete_dev, d, Mp);
    for (int i0 = 0; i0 < n; i0 += group) {
        const int cnt = std::min(group, n - i0);
        ++c->set_launches;
        if (!pre) {
            hipLaunchKernelGGL(predict_kernel_set<G>, dim3(tiles, cnt), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, dsets + i0, g0->ld, Np, g0->N, d,
                               Mp, g0->kernel, (double*)c->vscratch.p, cd->M);
            if (after_group && (rc = (*after_group)(i0, cnt)) != BOSS_OK) return rc;
            continue;
        }
        ++c->set_pre_launches;
        if (g0->kprog)
            kprog_kstar_set_launch(g0, cd, dsets + i0, tiles, cnt, (double*)c->vscratch.p, kpv + (size_t)i0 * Mp, (size_t)Mp, s);
        else if (g0->aug)
            hipLaunchKernelGGL(aug_kstar_set_kernel, dim3(Np / 256, tiles, cnt), dim3(256), sizeof(double) * ((size_t)d * (G::BN + 256) + d), s,
                               g0->ldx, d, g0->nhead, g0->N, Np, (const double*)cd->Craw, Mp, g0->kernel, dsets + i0,
                               (double*)c->vscratch.p, (int)G::BN);
        else
            hipLaunchKernelGGL(gibbs_kstar_set_kernel, dim3(Np / 256, tiles, cnt), dim3(256), sizeof(double) * (2 * d * 32 + 32 + 2 * 8 * 256), s,
                               d, g0->N, Np, (const double*)cd->Craw, Mp, dsets + i0, (double*)c->vscratch.p);
        // (a program kernel's epilogue is the nonstationary one, variance mode 2, as in predict_enqueue: KERN_PROGRAM never reaches kappa_*)
        hipLaunchKernelGGL((predict_kernel_set<G, true>), dim3(tiles, cnt), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, dsets + i0, g0->ld, Np,
                           g0->N, d, Mp, g0->kprog ? KERN_GIBBS : g0->kernel, (double*)c->vscratch.p, cd->M);
        if (g0->gibbs) hipLaunchKernelGGL(gibbs_var_set_kernel, dim3((cd->M + 255) / 256, cnt), dim3(256), 0, s, dsets + i0, cd->M);
        if (g0->kprog) kprog_var_set_launch(s, dsets + i0, cnt, kpv + (size_t)i0 * Mp, (size_t)Mp, cd->M);
        if (after_group && (rc = (*after_group)(i0, cnt)) != BOSS_OK) return rc;
    }
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

extern "C" int boss_gp_predict(boss_gp_t* g, int M, const double* Xs, const double* mean_Xs, double* mu, double* var,
                               long* bad_index) {
    if (!g || !Xs || !mu || !var) return fail(BOSS_E_INVALID, "NULL argument");
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (bad_index) *bad_index = -1;
    if (g->aug && mean_Xs) return fail(BOSS_E_INVALID, "gradient-observation posteriors take no prior mean (gradient_gp.jl:334-337)");
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);                 // the per-device scratch areas are shared
    {
        // one to four candidates on resident inverse factors: candidates in the kernel arguments, results polled in mapped memory
        const size_t winv_lds = sizeof(double) * (size_t)g->Np * (M == 1 ? 1 : M == 2 ? 2 : WINV_MAX_M);
        if (!few_args_off() && M <= WINV_MAX_M && g->have_winv && !g->pending && !g->aug && !g->gibbs && !g->kprog && g->d <= FEW_ARGS_MAX_D && !c->prof_on &&
            winv_lds <= 144 * 1024 && g->N > SMALL_MAX_N) {
            hipStream_t s = c->stream;
            const int nwg = g->Np / WINV_ROWS;
            int rc = ws_reserve(c->few, sizeof(double) * ((size_t)g->Np * 32 + 64 + (size_t)nwg * 8));
            if (rc) return rc;
            double* R = (double*)c->few.p;
            double* part = R + (size_t)g->Np * 32 + 64;
            FewCand par;
            par.ncols = M;
            for (int j = 0; j < WINV_MAX_M; ++j) {
                for (int k = 0; k < FEW_ARGS_MAX_D; ++k) {
                    double v = 0.0;
                    if (j < M && k < g->d) {
                        v = Xs[(size_t)j * g->d + k];
                        if (!g->discrete.empty() && g->discrete[k]) v = std::nearbyint(v);   // DiscreteKernel (kernels.jl:56-59)
                        v *= g->host_par[k];                                                   // 1/(λ + 1e-8) of the last update
                    }
                    par.x[j][k] = v;
                }
                par.mean[j] = (j < M && mean_Xs) ? mean_Xs[j] : 0.0;
            }
            g->dinv_used = true;                             // (the next update keeps the side-stream inverses coming, as after any prediction)
            double* hres = (double*)c->pinned + FEW_RES_OFF;
            const unsigned long long seq = ++c->few_seq;
            const int mc = M == 1 ? 1 : M == 2 ? 2 : 4;
            const bool fused = few_fused() && few_done_ensure(c, s);
            if (fused) {
                // ONE launch: K* rows, the pass over L⁻ᵀ, and the last workgroup's reduction into mapped host memory (small_calls.hpp)
                auto kfn = mc == 1 ? winv_args_kernel<1> : mc == 2 ? winv_args_kernel<2> : winv_args_kernel<4>;
                c->few_done_cnt += (unsigned long long)nwg;
                const size_t lds = sizeof(double) * std::max((size_t)g->Np * mc, (size_t)(8 * 256 + 64));
                const double* kst = nullptr;
                if (mc == 1) {
                    hipLaunchKernelGGL(kstar_args_kernel, dim3(g->Np / 256), dim3(256), 0, s, par, (const double*)g->Xsc, g->Np, g->N, g->d, g->kernel, g->amp2, R, 1);
                    kst = R;
                }
                hipLaunchKernelGGL(kfn, dim3(nwg), dim3(256), lds, s, par, (const double*)g->Xsc, g->N, g->d, g->kernel, g->amp2, (const double*)g->Winv,
                                   g->ld, g->Np, (const double*)g->A, g->ld, kst, part, c->few_done, c->few_done_cnt, hres, seq, AppendTail());
            } else {
                hipLaunchKernelGGL(kstar_args_kernel, dim3(g->Np / 256), dim3(256), 0, s, par, (const double*)g->Xsc, g->Np, g->N, g->d, g->kernel, g->amp2, R);
                auto kfn = mc == 1 ? winv_gemv_kernel<1> : mc == 2 ? winv_gemv_kernel<2> : winv_gemv_kernel<4>;
                hipLaunchKernelGGL(kfn, dim3(nwg), dim3(256), sizeof(double) * (size_t)g->Np * mc, s, (const double*)g->Winv, g->ld, g->Np,
                                   (const double*)g->A, g->ld, (const double*)R, M, part, (double*)nullptr);
                hipLaunchKernelGGL(winv_finish_host_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nwg, par, g->amp2, hres, seq);
            }
            volatile unsigned long long* sw = reinterpret_cast<volatile unsigned long long*>(hres) + 9;
            bool got = false;
            for (unsigned long i = 1;; ++i) {
                if (*sw == seq) {
                    got = true;
                    break;
                }
                if ((i & 0x3fff) == 0 && hipStreamQuery(s) != hipErrorNotReady) break;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            if (!got) {
                HIPCHK(hipStreamSynchronize(s));
                if (*sw != seq) {
                    // the stream drained without the answer (a launch of this call or of an earlier one did not run): the finished-workgroup
                    // counter no longer matches the host's — start it over rather than hand out the previous call's numbers
                    if (c->few_done) (void)hipMemset(c->few_done, 0, sizeof(unsigned long long));
                    c->few_done_cnt = 0;
                    HIPCHK(hipGetLastError());
                    return fail(BOSS_E_NO_DEVICE, "prediction kernel did not deliver its result (device error)");
                }
            }
            HIPCHK(hipGetLastError());
            for (int j = 0; j < M; ++j) {
                mu[j] = hres[j];
                var[j] = hres[4 + j];
            }
            long long bad;
            std::memcpy(&bad, &hres[8], sizeof bad);
            return bad >= 0 ? neg_var_error(bad_index, (unsigned long long)bad, var[bad]) : BOSS_OK;
        }
    }
    boss_cand cd;
    int rc = temp_cand(c, g->d, M, Xs, &cd);
    if (rc) return drain(c, rc);
    rc = ws_reserve(c->pred, sizeof(double) * (3 * (size_t)M + 2));   // mu | var | bad | mean
    if (rc) return drain(c, rc);
    double* dev = (double*)c->pred.p;
    double *dmu = dev, *dvar = dev + M, *dmean = dev + 2 * (size_t)M + 1;
    unsigned long long* dbad = (unsigned long long*)(dev + 2 * (size_t)M);
    hipStream_t s = c->stream;
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s);
    (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
    rc = predict_enqueue(g, &cd, mean_Xs ? dmean : nullptr, dmu, dvar);
    if (rc) return drain(c, rc);
    hipLaunchKernelGGL(clip_var_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dvar, M, dbad);
    unsigned long long bad = 0;
    rc = finish(c, {{mu, dmu, sizeof(double) * M}, {var, dvar, sizeof(double) * M}, {&bad, dbad, sizeof bad}});
    if (rc) return rc;
    return bad != ~0ULL ? neg_var_error(bad_index, bad, var[bad]) : BOSS_OK;
}

// mean_and_var of a NonstationaryGP posterior (GaussianProcessPosterior over the Gibbs kernel,
// nonstationary_gp.jl:153-157 -> gaussian_process.jl:143-194): lam_Xs d×M and amp_Xs M are the caller's latent
// models at the candidates (evaluated at the ROUNDED candidate where dims are discrete, as DiscreteKernel does).
// The candidates of a nonstationary call with the caller's λ(x*) (d×M) and α(x*) (M), checked and packed on the host (no device
// work): points rounded where dims are discrete, all three column-padded to Mp.
constexpr long long NGP_GRAD_SET_MAX_JAC = 1LL << 27;       // n·M·d² doubles of ∂λ/∂x (1 GiB) per call
struct NgpCand {
    int Mp = 0;
    std::vector<double> x, lam, amp;
};
static int ngp_pack(const boss_gp* g, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs, NgpCand& p) {
    const int d = g->d, Mp = round_up(M, 64);
    p.Mp = Mp;
    p.lam.assign((size_t)d * Mp, 1.0);
    p.amp.assign(Mp, 0.0);
    for (int j = 0; j < M; ++j) {
        for (int k = 0; k < d; ++k) {
            const double v = lam_Xs[(size_t)j * d + k];
            if (!(v > 0.0) || !std::isfinite(v)) return fail(BOSS_E_INVALID, "lengthscales must be finite and > 0");
            p.lam[(size_t)k * Mp + j] = v;
        }
        if (!(amp_Xs[j] >= 0.0) || !std::isfinite(amp_Xs[j])) return fail(BOSS_E_INVALID, "amplitudes must be finite and >= 0");
        p.amp[j] = amp_Xs[j];
    }
    pack_points(p.x, Xs, d, M, Mp, g->discrete.empty() ? nullptr : g->discrete.data());
    return BOSS_OK;
}
// The _lat calls pack the points alone: λ(x*), α(x*) come from the latent kernel.
static void ngp_pack_x(const boss_gp* g, int M, const double* Xs, NgpCand& p) {
    p.Mp = round_up(M, 64);
    pack_points(p.x, Xs, g->d, M, p.Mp, g->discrete.empty() ? nullptr : g->discrete.data());
}
// ... and uploaded into the per-device candidate workspace (Craw | λ | α).  Caller holds the context lock.
// lat: the λ and α buffers are filled by the latent kernel instead (Craw | λ | α | flag | ∂λ/∂x | ∂α/∂x; the Jacobians where djl
// is given); the call returns once the kernel's validity flag has been read (BOSS_E_INVALID: nothing stays enqueued).
static int ngp_upload(Ctx* c, int d, int M, const NgpCand& p, boss_cand& cd, double*& clam, double*& camp,
                      const boss_nlat_t* lat = nullptr, double** djl = nullptr, double** dja = nullptr) {
    const int Mp = p.Mp;
    hipStream_t s = c->stream;
    const size_t dm = (size_t)d * M;
    int rc = ws_reserve(c->craw, sizeof(double) * ((size_t)2 * d * Mp + Mp + (lat ? 1 + (djl ? dm * d + dm : 0) : 0)));
    if (rc) return rc;
    if (lat) {
        cd.ctx = c;
        cd.d = d;
        cd.M = M;
        cd.Mp = Mp;
        cd.Craw = (double*)c->craw.p;
        clam = cd.Craw + (size_t)d * Mp;
        camp = clam + (size_t)d * Mp;
        unsigned long long* dbad = (unsigned long long*)(camp + Mp);
        if (djl) {
            *djl = camp + Mp + 1;
            *dja = *djl + dm * d;
        }
        HIPCHK(hipMemcpyAsync(cd.Craw, p.x.data(), sizeof(double) * d * Mp, hipMemcpyHostToDevice, s));
        boss_nlat_t* one = const_cast<boss_nlat_t*>(lat);
        rc = nlat_enqueue(c, 1, &one, cd.Craw, Mp, M, clam, 0, camp, 0, djl ? *djl : nullptr, 0, djl ? *dja : nullptr, 0, nullptr, dbad);
        return rc ? rc : nlat_check(c, dbad, nullptr);
    }
    cd.ctx = c;
    cd.d = d;
    cd.M = M;
    cd.Mp = Mp;
    cd.Craw = (double*)c->craw.p;
    clam = cd.Craw + (size_t)d * Mp;
    camp = clam + (size_t)d * Mp;
    HIPCHK(hipMemcpyAsync(cd.Craw, p.x.data(), sizeof(double) * d * Mp, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(clam, p.lam.data(), sizeof(double) * d * Mp, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(camp, p.amp.data(), sizeof(double) * Mp, hipMemcpyHostToDevice, s));
    return BOSS_OK;
}

// (lat: the latent values come from a resident latent object — boss_ngp_predict_lat — instead of lam_Xs / amp_Xs)
static int ngp_predict_call(boss_gp_t* g, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs, const boss_nlat_t* lat,
                            const double* mean_Xs, double* mu, double* var, long* bad_index) {
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (bad_index) *bad_index = -1;
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    NgpCand pk;
    int rc = BOSS_OK;
    if (lat) {
        boss_nlat_t* one = const_cast<boss_nlat_t*>(lat);
        if ((rc = nlat_match(1, &g, &one)) != BOSS_OK) return rc;
        ngp_pack_x(g, M, Xs, pk);
    } else {
        rc = ngp_pack(g, M, Xs, lam_Xs, amp_Xs, pk);
    }
    if (rc) return rc;
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    boss_cand cd;
    double *clam, *camp;
    rc = ngp_upload(c, g->d, M, pk, cd, clam, camp, lat);
    if (rc) return drain(c, rc);
    rc = ws_reserve(c->pred, sizeof(double) * (3 * (size_t)M + 2));   // mu | var | bad | mean
    if (rc) return drain(c, rc);
    double* dev = (double*)c->pred.p;
    double *dmu = dev, *dvar = dev + M, *dmean = dev + 2 * (size_t)M + 1;
    unsigned long long* dbad = (unsigned long long*)(dev + 2 * (size_t)M);
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s);
    (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
    rc = predict_enqueue(g, &cd, mean_Xs ? dmean : nullptr, dmu, dvar, false, clam, camp);
    if (rc) return drain(c, rc);
    hipLaunchKernelGGL(clip_var_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dvar, M, dbad);
    unsigned long long bad = 0;
    rc = finish(c, {{mu, dmu, sizeof(double) * M}, {var, dvar, sizeof(double) * M}, {&bad, dbad, sizeof bad}});
    if (rc) return rc;
    return bad != ~0ULL ? neg_var_error(bad_index, bad, var[bad]) : BOSS_OK;
}
extern "C" int boss_ngp_predict(boss_gp_t* g, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                                const double* mean_Xs, double* mu, double* var, long* bad_index) {
    if (!g || !Xs || !lam_Xs || !amp_Xs || !mu || !var) return fail(BOSS_E_INVALID, "NULL argument");
    return ngp_predict_call(g, M, Xs, lam_Xs, amp_Xs, nullptr, mean_Xs, mu, var, bad_index);
}
extern "C" int boss_ngp_predict_lat(boss_gp_t* g, int M, const double* Xs, const boss_nlat_t* lat, const double* mean_Xs, double* mu,
                                    double* var, long* bad_index) {
    if (!g || !Xs || !lat || !mu || !var) return fail(BOSS_E_INVALID, "NULL argument");
    return ngp_predict_call(g, M, Xs, nullptr, nullptr, lat, mean_Xs, mu, var, bad_index);
}

// EI parameters: by value in the kernel arguments for P <= EI_MAXP, else in device arrays.
static int ei_params(Ctx* c, hipStream_t s, int P, const double* fit_coefs, const double* y_max, int has_best, double best,
                     EiPar* par, double* dcoef, double* dymax) {
    par->P = P;
    par->mode = (has_best ? 1 : 0) | (y_max ? 2 : 0);
    par->best = best;
    if (P <= EI_MAXP) {
        for (int p = 0; p < P; ++p) {
            par->coefs[p] = fit_coefs[p];
            par->ymax[p] = y_max ? y_max[p] : std::numeric_limits<double>::infinity();
        }
    } else {
        HIPCHK(hipMemcpyAsync(dcoef, fit_coefs, sizeof(double) * P, hipMemcpyHostToDevice, s));
        if (y_max) HIPCHK(hipMemcpyAsync(dymax, y_max, sizeof(double) * P, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return BOSS_OK;
}

// The two epilogues every acquisition call ends in, on device-resident moments (coef / ymax: ei_params' device arrays, read for
// P > EI_MAXP only; mask or null; mc or null: the EI term is the Monte-Carlo mean of a fitness program, deps its ε on the device).
// Value and gradient from mu / var [s][p][M], gm / gv [s][p][d×M].  single: one sample through ei_grad_kernel — the caller says
// so, because ei_grad_set_kernel with S = 1 adds the sample to 0.0 and is not the same bits (0.0 + (−0.0)).
static void ei_grad_epilogue_launch(hipStream_t s, const double* mu, const double* var, const double* gm, const double* gv, int M, int d, int S,
                                    bool single, const EiPar& par, const double* coef, const double* ymax, const unsigned char* mask,
                                    const McEpi* mc, const double* deps, double* acq, double* dacq, const AcqpEpi* pg = nullptr) {
    if (pg)                                                  // an acquisition program: value and chain rule of all S samples in its own kernel
        acqp_grad_launch(s, mu, var, gm, gv, M, d, S, *pg, mask, acq, dacq);
    else if (mc)
        mc_grad_launch(s, mu, var, gm, gv, M, d, S, par, *mc, deps, mask, acq, dacq);
    else if (single)
        hipLaunchKernelGGL(ei_grad_kernel, dim3((M + 127) / 128), dim3(128), 0, s, mu, var, gm, gv, M, d, par, coef, ymax, mask, acq, dacq);
    else
        hipLaunchKernelGGL(ei_grad_set_kernel, dim3((M + 127) / 128), dim3(128), 0, s, mu, var, gm, gv, M, d, S, par, coef, ymax, mask, acq, dacq);
}
// Value, mask and arg-max from mu / var [s][p][M]: samples 0 … S−2 summed into acq in sample order, the last one with the mean,
// the mask and the arg-max (into hres; res_seq, dpair, idx_off: acq_epilogue_kernel's).  mc: the Monte-Carlo sums of all S samples,
// then the epilogue in mode 0 (it adds 0.0 to them).  pg: the sums of an acquisition program, taken as they are (have_prev = 2) and
// masked to pg->outside.
static void ei_value_epilogue_launch(hipStream_t s, const double* mu, const double* var, int M, int S, const EiPar& par, const double* coef,
                                     const double* ymax, const unsigned char* mask, const McEpi* mc, const double* deps, double* acq,
                                     double* hres, unsigned long long res_seq, double* dpair = nullptr, long idx_off = 0,
                                     const AcqpEpi* pg = nullptr) {
    const size_t pm = (size_t)par.P * M;
    EiPar last = par;
    if (pg) {
        acqp_accumulate_launch(s, mu, var, pm, M, M, 0, S, *pg, acq, 0);
        last.mode = 0;
    } else if (mc) {
        mc_accumulate_launch(s, mu, var, pm, M, M, 0, S, S, par, *mc, deps, acq, 0);
        last.mode = 0;
    } else if (S > 1) {
        (void)hipMemsetAsync(acq, 0, sizeof(double) * M, s);
        hipLaunchKernelGGL(ei_accumulate_set_kernel, dim3((M + 255) / 256), dim3(256), 0, s, mu, var, pm, M, M, 0, S - 1, par, coef, ymax, acq);
    }
    hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, mu + pm * (S - 1), var + pm * (S - 1), M, M, last, coef, ymax,
                       acq, pg ? 2 : (mc || S > 1 ? 1 : 0), 1.0 / S, mask, hres, res_seq, dpair, idx_off, pg ? pg->outside : 0.0);
}

// SURVEY §8f3.  Enqueue μ, σ² (unclipped) and ∇μ, ∇σ² of one posterior at resident candidates:
// forward substitution (prediction kernel, 32-wide V slabs), adjoint substitution in place, gradient
// accumulation.  The transposed factor, the transposed 256×256 inverses and a = L⁻ᵀz are built once
// per factorisation.  mean_s_dev / mean_grad_dev may be null.
// Nonstationary posteriors: clam_dev / camp_dev are λ(x*), α(x*) on the device; the accumulation leaves its sums in gibbs_sums
// ([2 (2 d + 1)][Mp], gibbs_grad_accum_kernel) and the caller folds the latent models' Jacobians in (dmu / dvar are not written).
static int grad_enqueue(boss_gp* g, const boss_cand* cd, const double* mean_s_dev, const double* mean_grad_dev, double* mu,
                        double* var, double* dmu, double* dvar, const double* clam_dev = nullptr, const double* camp_dev = nullptr,
                        double* gibbs_sums = nullptr) {
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    const int d = g->d, Np = g->Np, M = cd->M;
    if (small_predict_ok(g, M)) {
        // N <= 128, few enough candidates (small_predict_ok): moments and gradients of all candidates in one launch
        // against L⁻¹ in LDS (small_predict_grad_kernel)
        if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
        if (cd->ctx != c) return fail(BOSS_E_INVALID, "candidates and posterior live on different devices");
        if (cd->d != d) return fail(BOSS_E_INVALID, "candidate dimension differs from the model's x_dim");
        small_dinv(g, s);
        const int grid = std::min(512, (M + SPG_WAVES - 1) / SPG_WAVES);
        hipLaunchKernelGGL(small_predict_grad_kernel<true>, dim3(grid), dim3(SPG_THREADS), SPG_LDS_BYTES, s, (const double*)g->Dinv,
                           (const double*)g->A, g->ld, Np, g->N, d, g->kernel, g->amp2, (const double*)g->Xsc, g->ldx,
                           (const double*)cd->Craw, cd->Mp, M, (const double*)g->invlam, (const unsigned char*)g->discrete_dev,
                           mean_s_dev, mean_grad_dev, mu, var, dmu, dvar);
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    }
    const size_t glds = sizeof(double) * ((size_t)d * GRAD_CHUNK + GRAD_CHUNK + 8 * 2 * (GRAD_MAX_D + 1) * 32);
    if (glds > 150 * 1024) return fail(BOSS_E_INVALID, "x_dim too large for the gradient kernel's LDS staging");
    int rc = lt_alloc(g);                                   // transposed factor, transposed inverses, a (host_latent.inc)
    if (rc) return rc;
    rc = predict_enqueue(g, cd, mean_s_dev, mu, var, true, clam_dev, camp_dev);    // V slabs (32 wide) + scaled candidates
    if (rc) return rc;
    lt_build(g, s);                                         // once per factorisation
    typedef PredG32 G;
    const int tiles = (M + 31) / 32;
    double* slabs = (double*)c->vscratch.p;
    if (tiles <= few_max_tiles() && tiles <= invgemm_max_tiles() && Np >= 4 * PRED_RB && !few_off() && g->have_winv) {
        // both inverse factors are resident (repeated calls on this factorisation): W = L⁻ᵀV as one GEMM
        typedef GemmDirect<4, 1, 2, 2, 8> GU;
        double* Wsl = slabs + (size_t)tiles * 32 * Np;
        hipLaunchKernelGGL(inv_bwd_kernel<GU>, dim3(tiles, Np / BLK), dim3(GU::NTHREADS), 0, s, (const double*)g->Winv, g->ld, Np,
                           (const double*)slabs, Wsl);
        slabs = Wsl;
    } else if (tiles <= few_max_tiles() && Np >= 4 * PRED_RB && !few_off()) {
        // few candidates: the adjoint substitution step by step across the chip (see few_back_* kernels)
        typedef GemmDirect<4, 1, 2, 2, 8> GU;
        for (int ib = Np / PRED_RB - 1; ib >= 0; --ib) {
            hipLaunchKernelGGL(few_back_finish_kernel<G>, dim3(tiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s,
                               (const double*)g->DT2, Np, ib, slabs);
            if (ib > 0)
                hipLaunchKernelGGL(few_back_update_kernel<GU>, dim3(tiles, ib * (PRED_RB / BLK)), dim3(GU::NTHREADS), 0, s,
                                   (const double*)g->LT, g->ld, Np, ib, slabs);
        }
    } else {
        hipLaunchKernelGGL(backsolve_kernel<G>, dim3(tiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, (const double*)g->LT,
                           g->ld, Np, (const double*)g->DT2, slabs);
    }
    if (g->gibbs) {
        hipLaunchKernelGGL(gibbs_grad_accum_kernel, dim3(tiles), dim3(256), 0, s, (const double*)slabs, (const double*)g->avec, Np, g->N,
                           (const double*)g->Xraw, (const double*)g->lamX, (const double*)g->ampX, (const double*)cd->Craw, clam_dev, camp_dev, d,
                           cd->Mp, (const unsigned char*)g->discrete_dev, gibbs_sums);
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    }
    if (g->aug) {
        // gradient observations: the rows are (derivative order, point) pairs, the accumulation walks the POINTS (aug_grad_accum_kernel)
        int rsp = std::max(1, std::min(32, std::min(512 / std::max(1, tiles), (g->npts + 63) / 64)));
        double* apart = nullptr;
        if (rsp > 1) {
            rc = ws_reserve(c->few, sizeof(double) * (size_t)tiles * std::max((size_t)Np * 32 + 64, (size_t)rsp * 2 * AUG_MAX_D * 32));
            if (rc) return rc;
            apart = (double*)c->few.p;                       // the forward pass's residuals are dead by now
        }
        hipLaunchKernelGGL(aug_grad_accum_kernel, dim3(tiles, rsp), dim3(256), 0, s, (const double*)slabs, (const double*)g->avec, Np, g->npts, g->nhead,
                           (const double*)g->Xraw, g->ldx, (const double*)cd->Craw, d, cd->Mp, M, g->kernel, g->amp2, (const double*)g->invlam,
                           dmu, dvar, apart);
        if (rsp > 1)
            hipLaunchKernelGGL(aug_grad_finalize_kernel, dim3(tiles), dim3(32), 0, s, (const double*)apart, rsp, d, M, g->amp2, dmu, dvar);
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    }
    if (g->kprog && d > GRAD_MAX_D) return fail(BOSS_E_INVALID, "x_dim too large for the program-kernel gradient kernel");
    // few tiles: split the rows of every tile over several workgroups (one workgroup per tile would walk all N rows alone)
    int rsplit = 1;
    if (d <= GRAD_MAX_D && tiles < 128) {
        rsplit = std::min(32, std::max(1, 512 / tiles));
        rsplit = std::min(rsplit, (g->N + GRAD_CHUNK - 1) / GRAD_CHUNK);
    }
    double* part = nullptr;
    if (rsplit > 1) {
        rc = ws_reserve(c->few, sizeof(double) * (size_t)tiles * std::max((size_t)Np * 32 + 64, (size_t)rsplit * 2 * (GRAD_MAX_D + 1) * 32));
        if (rc) return rc;
        part = (double*)c->few.p;                          // the forward pass's residuals are dead by now
    }
    if (g->kprog)
        kprog_grad_accum_launch(g, cd, s, tiles, rsplit, slabs, (const double*)c->csc.p, mean_grad_dev, dmu, dvar, part);
    else
    hipLaunchKernelGGL(grad_accum_kernel, dim3(tiles, rsplit), dim3(256), glds, s, (const double*)slabs, (const double*)g->avec, Np,
                       g->N, (const double*)g->Xsc, (const double*)c->csc.p, d, cd->Mp, M, g->kernel, g->amp2,
                       (const double*)g->invlam, (const unsigned char*)g->discrete_dev, mean_grad_dev, dmu, dvar, part);
    if (rsplit > 1)
        hipLaunchKernelGGL(grad_finalize_kernel, dim3(tiles), dim3(32), 0, s, (const double*)part, rsplit, (const double*)c->csc.p, d,
                           cd->Mp, M, (const double*)g->invlam, (const unsigned char*)g->discrete_dev, mean_grad_dev, dmu, dvar);
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

extern "C" int boss_gp_predict_grad(boss_gp_t* g, int M, const double* Xs, const double* mean_Xs, const double* mean_grad,
                                    double* mu, double* var, double* dmu, double* dvar, long* bad_index) {
    if (!g || !Xs || !mu || !var || !dmu || !dvar) return fail(BOSS_E_INVALID, "NULL argument");
    KPROG_NEEDS_GRAD(g);
    NOT_FOR_GIBBS_MODEL(g, mean_Xs, mean_grad);
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (bad_index) *bad_index = -1;
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    boss_cand cd;
    int rc = temp_cand(c, g->d, M, Xs, &cd);
    if (rc) return drain(c, rc);
    const int d = g->d;
    const size_t dm = (size_t)d * M;
    rc = ws_reserve(c->pred, sizeof(double) * (3 * (size_t)M + 3 * dm + 2));   // mu | var | dmu | dvar | bad | mean | mean_grad
    if (rc) return drain(c, rc);
    double* dev = (double*)c->pred.p;
    double *dmu_ = dev, *dvar_ = dev + M, *dgm = dev + 2 * (size_t)M, *dgv = dgm + dm;
    unsigned long long* dbad = (unsigned long long*)(dgv + dm);
    double *dmean = dgv + dm + 1, *dmg = dmean + M;
    hipStream_t s = c->stream;
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s);
    if (mean_grad) (void)hipMemcpyAsync(dmg, mean_grad, sizeof(double) * dm, hipMemcpyHostToDevice, s);
    (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
    rc = grad_enqueue(g, &cd, mean_Xs ? dmean : nullptr, mean_grad ? dmg : nullptr, dmu_, dvar_, dgm, dgv);
    if (rc) return drain(c, rc);
    hipLaunchKernelGGL(clip_var_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dvar_, M, dbad);
    unsigned long long bad = 0;
    rc = finish(c, {{mu, dmu_, sizeof(double) * M}, {var, dvar_, sizeof(double) * M}, {dmu, dgm, sizeof(double) * dm},
                    {dvar, dgv, sizeof(double) * dm}, {&bad, dbad, sizeof bad}});
    if (rc) return rc;
    return bad != ~0ULL ? neg_var_error(bad_index, bad, var[bad]) : BOSS_OK;
}

// mean_and_var of a NonstationaryGP posterior AND its gradient w.r.t. the candidates: what ForwardDiff pushes through
// nonstationary_gp.jl:153-196 inside OptimizationAM (src/acquisition_maximizers/optimization.jl:36,89-118).  The candidate enters the
// Gibbs kernel directly and through the latent λ(x*), α(x*): their Jacobians arrive evaluated, like their values —
//   dlam_Xs d×d×M, dlam_Xs[l + d (m + d j)] = ∂λ_l/∂x_m at candidate j (NULL: constant λ);  damp_Xs d×M (NULL: constant α).
// The device accumulates Σ_i a_i k_i ∇ln k_i and Σ_i w_i k_i ∇ln k_i in their three parts (explicit, through λ*, through α*:
// gibbs_grad_accum_kernel), the Jacobians are folded in here (M d² multiply-adds).
// (lat: values and Jacobians come from a resident latent object — boss_ngp_predict_grad_lat —, are folded in by the same host
// loop and therefore come back with the sums)
static int ngp_predict_grad_call(boss_gp_t* g, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                                 const double* dlam_Xs, const double* damp_Xs, const boss_nlat_t* lat, const double* mean_Xs,
                                 const double* mean_grad, double* mu, double* var, double* dmu, double* dvar, long* bad_index) {
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (g->d > GIBBS_GRAD_MAX_D) return fail(BOSS_E_INVALID, "x_dim above 16 is not supported by the nonstationary gradient kernel");
    if (bad_index) *bad_index = -1;
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    NgpCand pk;
    int rc = BOSS_OK;
    if (lat) {
        boss_nlat_t* one = const_cast<boss_nlat_t*>(lat);
        if ((rc = nlat_match(1, &g, &one)) != BOSS_OK) return rc;
        if ((long long)M * g->d * g->d > NGP_GRAD_SET_MAX_JAC) return fail(BOSS_E_INVALID, "M·x_dim² above 2^27 is not supported");
        ngp_pack_x(g, M, Xs, pk);
    } else {
        rc = ngp_pack(g, M, Xs, lam_Xs, amp_Xs, pk);
    }
    if (rc) return rc;
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    boss_cand cd;
    double *clam, *camp, *djl = nullptr, *dja = nullptr;
    rc = ngp_upload(c, g->d, M, pk, cd, clam, camp, lat, &djl, &dja);
    if (rc) return drain(c, rc);
    const int d = g->d, Mp = pk.Mp, nslot = 2 * (2 * d + 1);
    const size_t nsums = (size_t)nslot * Mp;
    rc = ws_reserve(c->pred, sizeof(double) * (3 * (size_t)M + 2 + nsums));   // mu | var | sums | bad | mean
    if (rc) return drain(c, rc);
    double* dev = (double*)c->pred.p;
    double *dmu_ = dev, *dvar_ = dev + M, *dsums = dev + 2 * (size_t)M, *dmean = dsums + nsums + 1;
    unsigned long long* dbad = (unsigned long long*)(dsums + nsums);
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s);
    (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
    rc = grad_enqueue(g, &cd, mean_Xs ? dmean : nullptr, nullptr, dmu_, dvar_, nullptr, nullptr, clam, camp, dsums);
    if (rc) return drain(c, rc);
    hipLaunchKernelGGL(clip_var_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dvar_, M, dbad);
    unsigned long long bad = 0;
    std::vector<double> sums(nsums), hjl, hja, hamp;
    if (lat) {
        const size_t dm = (size_t)d * M;
        hjl.resize(dm * d);
        hja.resize(dm);
        hamp.resize(M);
        rc = finish(c, {{mu, dmu_, sizeof(double) * M}, {var, dvar_, sizeof(double) * M}, {sums.data(), dsums, sizeof(double) * nsums},
                        {&bad, dbad, sizeof bad}, {hjl.data(), djl, sizeof(double) * dm * d}, {hja.data(), dja, sizeof(double) * dm},
                        {hamp.data(), camp, sizeof(double) * M}});
        dlam_Xs = hjl.data();
        damp_Xs = hja.data();
        amp_Xs = hamp.data();
    } else {
        rc = finish(c, {{mu, dmu_, sizeof(double) * M}, {var, dvar_, sizeof(double) * M}, {sums.data(), dsums, sizeof(double) * nsums},
                        {&bad, dbad, sizeof bad}});
    }
    if (rc) return rc;
    const int ns1 = 2 * d + 1;
    for (int j = 0; j < M; ++j) {
        const double* Dl = dlam_Xs ? dlam_Xs + (size_t)j * d * d : nullptr;
        const double* Da = damp_Xs ? damp_Xs + (size_t)j * d : nullptr;
        for (int m = 0; m < d; ++m) {
            double ga = sums[(size_t)(1 + m) * Mp + j], gw = sums[(size_t)(ns1 + 1 + m) * Mp + j];
            if (Dl)
                for (int l = 0; l < d; ++l) {
                    ga += Dl[l + (size_t)d * m] * sums[(size_t)(1 + d + l) * Mp + j];
                    gw += Dl[l + (size_t)d * m] * sums[(size_t)(ns1 + 1 + d + l) * Mp + j];
                }
            double av = 0.0;
            if (Da) {
                ga += Da[m] * sums[j];
                gw += Da[m] * sums[(size_t)ns1 * Mp + j];
                av = 2.0 * amp_Xs[j] * Da[m];
            }
            dmu[(size_t)j * d + m] = ga + (mean_grad ? mean_grad[(size_t)j * d + m] : 0.0);
            dvar[(size_t)j * d + m] = av - 2.0 * gw;
        }
    }
    return bad != ~0ULL ? neg_var_error(bad_index, bad, var[bad]) : BOSS_OK;
}
extern "C" int boss_ngp_predict_grad(boss_gp_t* g, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                                     const double* dlam_Xs, const double* damp_Xs, const double* mean_Xs, const double* mean_grad,
                                     double* mu, double* var, double* dmu, double* dvar, long* bad_index) {
    if (!g || !Xs || !lam_Xs || !amp_Xs || !mu || !var || !dmu || !dvar) return fail(BOSS_E_INVALID, "NULL argument");
    return ngp_predict_grad_call(g, M, Xs, lam_Xs, amp_Xs, dlam_Xs, damp_Xs, nullptr, mean_Xs, mean_grad, mu, var, dmu, dvar, bad_index);
}
extern "C" int boss_ngp_predict_grad_lat(boss_gp_t* g, int M, const double* Xs, const boss_nlat_t* lat, const double* mean_Xs,
                                         const double* mean_grad, double* mu, double* var, double* dmu, double* dvar, long* bad_index) {
    if (!g || !Xs || !lat || !mu || !var || !dmu || !dvar) return fail(BOSS_E_INVALID, "NULL argument");
    return ngp_predict_grad_call(g, M, Xs, nullptr, nullptr, nullptr, nullptr, lat, mean_Xs, mean_grad, mu, var, dmu, dvar, bad_index);
}

// ------------------------------------------------------------------------------------------
// Moments AND moment gradients of a SET of equally shaped posteriors at the same candidates (boss_acq_ei_grad_set): the forward
// substitution of all members through predict_set_enqueue, and behind every group of members the adjoint substitution
// (backsolve_set_kernel, grid = tiles × members) and the accumulation (grad_accum_set_kernel / aug_grad_accum_set_kernel).
// ------------------------------------------------------------------------------------------
static bool grad_set_ok(int n, boss_gp_t* const* gps, const boss_cand* cd) {
    if (!predict_set_ok(n, gps, cd)) return false;
    const boss_gp* g0 = gps[0];
    // (N <= 128 with few candidates: the one-launch small_predict_grad_kernel of grad_enqueue is the better path)
    return !g0->gibbs && !g0->kprog && !small_predict_ok(g0, cd->M) && (!g0->aug || g0->d <= AUG_MAX_D);
}

// mu / var of member i at mu_all + i·M (unclipped), ∇μ / ∇σ² at gm_all + i·d·M; mean_all / mg_all (or null): the prior means and
// their gradients in the same layouts.  Caller holds the context lock and has checked grad_set_ok.  BOSS_E_ALLOC: nothing the
// caller relies on has been written (what was enqueued is overwritten by the member-by-member path the caller turns to).
// Nonstationary members (ngp_grad_set_ok): clam_all / camp_all as predict_set_enqueue takes them, dlam_all [n][M][d×d] / damp_all
// [n][M][d] (or null) the latent models' Jacobians; the accumulation leaves partial sums and gibbs_grad_fold_set_kernel folds the
// Jacobians in on the device.
static int grad_set_enqueue(int n, boss_gp_t* const* gps, const boss_cand* cd, const double* mean_all, const double* mg_all,
                            double* mu_all, double* var_all, double* gm_all, double* gv_all, const double* clam_all = nullptr,
                            const double* camp_all = nullptr, const double* dlam_all = nullptr, const double* damp_all = nullptr) {
    boss_gp* g0 = gps[0];
    Ctx* c = g0->ctx;
    hipStream_t s = c->stream;
    typedef PredG32 G;
    const int d = g0->d, Np = g0->Np, ld = g0->ld, M = cd->M, Mp = cd->Mp;
    const int tiles = (M + 31) / 32, nb = Np / PRED_RB;
    const size_t dm = (size_t)d * M;
    const size_t glds = sizeof(double) * ((size_t)d * GRAD_CHUNK + GRAD_CHUNK + 8 * 2 * (GRAD_MAX_D + 1) * 32);
    if (!g0->aug && glds > 150 * 1024) return fail(BOSS_E_INVALID, "x_dim too large for the gradient kernel's LDS staging");
    std::vector<int> prep;                                   // members whose transposed factor is not current
    for (int i = 0; i < n; ++i) {
        boss_gp* g = gps[i];
        if (!g->LT) {
            if (dev_malloc((void**)&g->LT, sizeof(double) * (size_t)ld * Np) != hipSuccess ||
                dev_malloc((void**)&g->DT2, sizeof(double) * (size_t)Np * PRED_RB) != hipSuccess ||
                dev_malloc((void**)&g->avec, sizeof(double) * (size_t)Np * 2) != hipSuccess) {
                if (g->LT) (void)hipFree(g->LT);
                if (g->DT2) (void)hipFree(g->DT2);
                g->LT = g->DT2 = g->avec = nullptr;
                (void)hipGetLastError();
                return fail(BOSS_E_ALLOC, "device allocation failed (transposed factor)");
            }
            g->have_lt = false;
        }
        if (!g->have_lt) prep.push_back(i);
    }
    // scratch whose addresses go into the descriptors, or that a later group must not move: reserved before anything is enqueued
    int rc = g0->aug || g0->gibbs ? BOSS_OK : ws_reserve(c->csc, sizeof(double) * (size_t)d * Mp * n);
    if (rc) return rc;
    const size_t part_one = (size_t)32 * (g0->aug ? 2 * AUG_MAX_D : g0->gibbs ? 2 * (2 * d + 1) : 2 * (GRAD_MAX_D + 1));   // doubles per (member, tile, split)
    // workgroups wanted in flight before the rows of a tile stop being split (BOSS_SET_GRAD_FILL overrides, 0: never split)
    static const int fill_env = getenv("BOSS_SET_GRAD_FILL") ? std::max(0, atoi(getenv("BOSS_SET_GRAD_FILL"))) : -1;
    const int fill = fill_env >= 0 ? fill_env : 2 * c->n_cus;
    rc = ws_reserve(c->few, sizeof(double) * part_one * std::max((size_t)fill, (size_t)n * tiles));
    if (rc) return rc;
    const size_t ndesc = (size_t)n + prep.size();
    rc = ws_reserve(c->gsetdesc, sizeof(GradSet) * ndesc);
    if (rc) return rc;
    std::vector<GradSet> desc(ndesc);
    for (int i = 0; i < n; ++i) {
        const boss_gp* g = gps[i];
        GradSet& q = desc[i];
        q.A = g->A;
        q.Dinv2 = g->Dinv2;
        q.LT = g->LT;
        q.DT2 = g->DT2;
        q.avec = g->avec;
        q.Xsc = g->Xsc;
        q.Xraw = g->Xraw;
        q.Csc = g0->aug || g0->gibbs ? nullptr : (const double*)c->csc.p + (size_t)i * d * Mp;   // (where predict_set_enqueue puts them)
        q.invlam = g->invlam;
        q.mean_grad = mg_all ? mg_all + (size_t)i * dm : nullptr;
        q.dmu = gm_all + (size_t)i * dm;
        q.dvar = gv_all + (size_t)i * dm;
        q.amp2 = g->amp2;
        if (g->gibbs) {
            q.lamX = g->lamX;
            q.ampX = g->ampX;
            q.clam = clam_all + (size_t)i * d * Mp;
            q.camp = camp_all + (size_t)i * Mp;
            q.dlam = dlam_all ? dlam_all + (size_t)i * d * dm : nullptr;
            q.damp = damp_all ? damp_all + (size_t)i * dm : nullptr;
        }
    }
    for (size_t k = 0; k < prep.size(); ++k) desc[n + k] = desc[prep[k]];
    const size_t dbytes = sizeof(GradSet) * ndesc;
    if (dbytes <= PINNED_UP_BYTES) {
        void* stage = (char*)c->pinned + PINNED_UP_OFF;
        HIPCHK(hipEventSynchronize(c->ev_up));               // (the candidates' upload out of the same area)
        std::memcpy(stage, desc.data(), dbytes);
        HIPCHK(hipMemcpyAsync(c->gsetdesc.p, stage, dbytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(c->ev_up, s));
    } else {
        HIPCHK(hipMemcpyAsync(c->gsetdesc.p, desc.data(), dbytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    const GradSet* gsets = (const GradSet*)c->gsetdesc.p;
    if (!prep.empty()) {
        // once per factorisation, for all members that need it together: LT, DT2 and a = L⁻ᵀz in 256-row steps from the last to the
        // first; grid.z of the DT2 transposition is member · nb + block, so at most 65535 / nb members per launch
        set_dinv_enqueue(n, gps, s);
        const int np = (int)prep.size(), chunk = 65535 / nb;
        for (int k0 = 0; k0 < np; k0 += chunk) {
            const int kc = std::min(chunk, np - k0);
            const GradSet* ps = gsets + n + k0;
            hipLaunchKernelGGL(transpose_set_kernel, dim3(Np / 64, Np / 64, kc), dim3(256), 0, s, ps, 0, ld, Np);
            hipLaunchKernelGGL(transpose_set_kernel, dim3(PRED_RB / 64, PRED_RB / 64, nb * kc), dim3(256), 0, s, ps, 1, ld, Np);
            for (int ib = nb - 1; ib >= 0; --ib) {
                const int nch = nb - 1 - ib;
                if (nch > 0) hipLaunchKernelGGL(bt_gemv_partial_set_kernel, dim3(nch, kc), dim3(256), 0, s, ps, ld, Np, ib);
                hipLaunchKernelGGL(bt_finish_set_kernel, dim3(1, kc), dim3(256), 0, s, ps, ld, Np, g0->N, ib, nch);
            }
        }
        HIPCHK(hipGetLastError());
        // (the launches are on the stream already: an error later in this call ends in drain(), which waits for them, so the arrays
        // are current whatever the call returns)
        for (int i : prep) gps[i]->have_lt = true;
    }
    std::function<int(int, int)> after = [&](int i0, int cnt) -> int {
        double* slabs = (double*)c->vscratch.p;
        ++c->set_grad_launches;
        hipLaunchKernelGGL(backsolve_set_kernel<G>, dim3(tiles, cnt), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, gsets + i0, ld, Np, slabs);
        // members × tiles fill the chip on their own from 2 workgroups per CU on; below that the rows of a tile are split as in grad_enqueue
        const int wgs = tiles * cnt;
        int rsplit = wgs >= fill ? 1 : std::min(32, std::max(1, fill / wgs));
        double* part = (double*)c->few.p;
        if (g0->gibbs) {
            // (always through the partial sums: the fold kernel reads them and writes the members' slices)
            rsplit = std::max(1, std::min(rsplit, (g0->N + GRAD_CHUNK - 1) / GRAD_CHUNK));
            auto kfn = d <= 4 ? gibbs_grad_accum_set_kernel<4> : d <= 8 ? gibbs_grad_accum_set_kernel<8> : gibbs_grad_accum_set_kernel<16>;
            hipLaunchKernelGGL(kfn, dim3(tiles, rsplit, cnt), dim3(256), 0, s, gsets + i0, (const double*)slabs, Np, g0->N,
                               (const double*)cd->Craw, d, Mp, (const unsigned char*)g0->discrete_dev, part);
            hipLaunchKernelGGL(gibbs_grad_fold_set_kernel, dim3(tiles, cnt), dim3(256), 0, s, gsets + i0, (const double*)part, rsplit, d, M);
        } else if (g0->aug) {
            rsplit = std::max(1, std::min(rsplit, (g0->npts + 63) / 64));
            hipLaunchKernelGGL(aug_grad_accum_set_kernel, dim3(tiles, rsplit, cnt), dim3(256), 0, s, gsets + i0, (const double*)slabs, Np, g0->npts, g0->nhead,
                               g0->ldx, (const double*)cd->Craw, d, Mp, M, g0->kernel, rsplit > 1 ? part : nullptr);
            if (rsplit > 1)
                hipLaunchKernelGGL(aug_grad_finalize_set_kernel, dim3(tiles, cnt), dim3(32), 0, s, gsets + i0, (const double*)part, rsplit, d, M);
        } else {
            if (d > GRAD_MAX_D) rsplit = 1;
            rsplit = std::max(1, std::min(rsplit, (g0->N + GRAD_CHUNK - 1) / GRAD_CHUNK));
            hipLaunchKernelGGL(grad_accum_set_kernel, dim3(tiles, rsplit, cnt), dim3(256), glds, s, gsets + i0, (const double*)slabs, Np, g0->N, d,
                               Mp, M, g0->kernel, (const unsigned char*)g0->discrete_dev, rsplit > 1 ? part : nullptr);
            if (rsplit > 1)
                hipLaunchKernelGGL(grad_finalize_set_kernel, dim3(tiles, cnt), dim3(32), 0, s, gsets + i0, (const double*)part, rsplit, d, Mp, M,
                                   (const unsigned char*)g0->discrete_dev);
        }
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    };
    return predict_set_enqueue(n, gps, cd, mean_all, mu_all, var_all, (size_t)M, clam_all, camp_all, &after);
}
static bool ngp_grad_set_ok(int n, boss_gp_t* const* gps, const boss_cand* cd) {
    return predict_set_ok(n, gps, cd, true) && gps[0]->d <= GIBBS_GRAD_MAX_D;
}

// ------------------------------------------------------------------------------------------
// The moments (and, with q.gm, their gradients) of n posteriors at one candidate set into device slices: THE place that chooses
// between the set launches and member by member, and the only loop over members, of every acquisition and set-prediction call
// (acq_ei_impl, host_acq.inc, keeps its own per-sample loop and asks members_set_path).  Enqueue only: the caller holds the
// context lock and drains on error.
// ------------------------------------------------------------------------------------------
struct MemberSlices {                                        // device pointers; member i at + i·M (moments) / + i·d·M (gradients)
    const double *mean = nullptr, *mean_grad = nullptr;      // prior means and their gradients, or null
    double *mu = nullptr, *var = nullptr, *gm = nullptr, *gv = nullptr;   // gm null: values only
    // nonstationary members: λ(x*) [n][d×Mp], α(x*) [n][Mp], their Jacobians [n][M][d×d] / [n][M][d] (or null), and the sums of ONE
    // member ([2 (2 d + 1)][Mp]) for the member-by-member gradient
    const double *clam = nullptr, *camp = nullptr, *dlam = nullptr, *damp = nullptr;
    double* sums = nullptr;
};
// allow_set: what the entry point permits; BOSS_NO_SET_PREDICT and the members' shapes decide the rest
static bool members_set_path(int n, boss_gp_t* const* gps, const boss_cand* cd, bool allow_set, bool grad, bool latents) {
    if (!allow_set || set_predict_off()) return false;
    return !grad ? predict_set_ok(n, gps, cd, latents) : latents ? ngp_grad_set_ok(n, gps, cd) : grad_set_ok(n, gps, cd);
}
static int members_enqueue(int n, boss_gp_t* const* gps, const boss_cand* cd, const MemberSlices& q, bool allow_set) {
    const int d = cd->d, M = cd->M, Mp = cd->Mp;
    const size_t dm = (size_t)d * M;
    if (members_set_path(n, gps, cd, allow_set, q.gm != nullptr, q.clam != nullptr)) {
        if (!q.gm) return predict_set_enqueue(n, gps, cd, q.mean, q.mu, q.var, (size_t)M, q.clam, q.camp);
        int rc = grad_set_enqueue(n, gps, cd, q.mean, q.mean_grad, q.mu, q.var, q.gm, q.gv, q.clam, q.camp, q.dlam, q.damp);
        if (rc != BOSS_E_ALLOC) return rc;                   // (no memory for the set launches: the call goes on member by member)
    }
    for (int i = 0; i < n; ++i) {
        const double *mean = q.mean ? q.mean + (size_t)i * M : nullptr, *mg = q.mean_grad ? q.mean_grad + (size_t)i * dm : nullptr;
        const double *cl = q.clam ? q.clam + (size_t)i * d * Mp : nullptr, *ca = q.clam ? q.camp + (size_t)i * Mp : nullptr;
        double *mu = q.mu + (size_t)i * M, *var = q.var + (size_t)i * M;
        int rc;
        if (!q.gm)
            rc = predict_enqueue(gps[i], cd, mean, mu, var, false, cl, ca);
        else if (!q.clam)
            rc = grad_enqueue(gps[i], cd, mean, mg, mu, var, q.gm + (size_t)i * dm, q.gv + (size_t)i * dm);
        else
            rc = grad_enqueue(gps[i], cd, mean, nullptr, mu, var, nullptr, nullptr, cl, ca, q.sums);
        if (rc) return rc;
        if (q.gm && q.clam)                                  // the latent models' Jacobians and the prior mean's gradient into the member's slices
            hipLaunchKernelGGL(gibbs_grad_fold_kernel, dim3((M + 31) / 32), dim3(256), 0, cd->ctx->stream, (const double*)q.sums, Mp,
                               q.dlam ? q.dlam + (size_t)i * d * dm : nullptr, q.damp ? q.damp + (size_t)i * dm : nullptr, ca, mg,
                               q.gm + (size_t)i * dm, q.gv + (size_t)i * dm, d, M);
    }
    return BOSS_OK;
}

// boss_acq_ei_grad averaged over S hyper-parameter samples in one call (expected_improvement.jl:87-90 inside the multistart
// refinement of optimization.jl:89-118): gps[p + P·s]; the candidates are uploaded once, every member's moments and moment
// gradients stay on the device ([s][p] slices), and ONE epilogue applies the chain rule per sample and sums in ascending s.
// Equally shaped members take the set launches, any other list goes member by member into the same slices (members_enqueue).
// S = 1 (boss_acq_ei_grad, one hyper-parameter sample): always member by member, and ei_grad_kernel.
// mc: the EI term and its gradient are those of a fitness program's Monte-Carlo mean (boss_acq_ei_mc_grad, host_fitness.inc); fit_coefs
// is not read, P <= EI_MAXP, and S = 1 may take the set launches too.  pg: an acquisition program's value and gradient instead
// (boss_acq_prog_grad, host_acqprog.inc); neither fit_coefs nor y_max / best is read, program-kernel handles are taken as for EI.
static int acq_ei_grad_set_impl(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best,
                                double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out, const McEpi* mc,
                                const AcqpEpi* pg = nullptr) {
    if (P < 1 || S < 1 || !gps || M < 1 || !Xs || (!fit_coefs && !mc && !pg) || !acq_out || !dacq_out) return fail(BOSS_E_INVALID, "bad arguments");
    if ((long long)P * S * M > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M above 2^30 is not supported");
    const int n = P * S;
    for (int i = 0; i < n; ++i) {
        if (!gps[i]) return fail(BOSS_E_INVALID, "NULL posterior handle");
        if (mc) NOT_FOR_KPROG(gps[i]);                       // (Monte-Carlo EI: built-in kernels only)
        KPROG_NEEDS_GRAD(gps[i]);                            // (flagged program handles go member by member: grad_set_ok)
        NOT_FOR_GIBBS_MODEL(gps[i], mean_Xs, mean_grad);
        if (gps[i]->ctx != gps[0]->ctx || gps[i]->d != gps[0]->d)
            return fail(BOSS_E_INVALID, "all handles must live on one device and share x_dim");
    }
    for (int i = 0; i < n; ++i)
        if (!gps[i]->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    Ctx* c = gps[0]->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    const int d = gps[0]->d;
    boss_cand cd;
    int rc = temp_cand(c, d, M, Xs, &cd);
    if (rc) return drain(c, rc);
    hipStream_t s = c->stream;
    const size_t dm = (size_t)d * M, nm = (size_t)n * M, ndm = (size_t)n * dm;
    // device scratch: acq[M] | dacq[dM] | mu[n][M] | var[n][M] | dmu[n][dM] | dvar[n][dM] | mean[n][M] | mean_grad[n][dM] | coefs[P] | ymax[P] | mask
    const size_t nd = M + dm + 3 * nm + 3 * ndm + 2 * (size_t)P;
    rc = ws_reserve(c->pred, sizeof(double) * nd + M);
    if (rc) return drain(c, rc);
    double* dacq = (double*)c->pred.p;
    double* ddacq = dacq + M;
    double* dmu = ddacq + dm;
    double* dvar = dmu + nm;
    double* dgm = dvar + nm;
    double* dgv = dgm + ndm;
    double* dmean = dgv + ndm;
    double* dmg = dmean + nm;
    double* dcoef = dmg + ndm;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(dacq + nd);
    EiPar par;
    const double no_coefs[EI_MAXP] = {};
    rc = ei_params(c, s, P, (mc || pg) ? no_coefs : fit_coefs, y_max, has_best, best, &par, dcoef, dymax);
    if (rc) return drain(c, rc);
    const double* deps = nullptr;
    if (mc) {
        rc = mc_stage(c, s, P, *mc, &deps);
        if (rc) return drain(c, rc);
    }
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * nm, hipMemcpyHostToDevice, s);
    if (mean_grad) (void)hipMemcpyAsync(dmg, mean_grad, sizeof(double) * ndm, hipMemcpyHostToDevice, s);
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    if (par.mode != 0) {
        MemberSlices q;
        q.mean = mean_Xs ? dmean : nullptr;
        q.mean_grad = mean_grad ? dmg : nullptr;
        q.mu = dmu, q.var = dvar, q.gm = dgm, q.gv = dgv;
        rc = members_enqueue(n, gps, &cd, q, mc || S > 1);
        if (rc) return drain(c, rc);
    }
    ei_grad_epilogue_launch(s, dmu, dvar, dgm, dgv, M, d, S, S == 1 && !mc, par, dcoef, dymax, valid_mask ? dmask : nullptr, mc, deps, dacq, ddacq, pg);
    return finish(c, {{acq_out, dacq, sizeof(double) * M}, {dacq_out, ddacq, sizeof(double) * dm}});
}

// Acquisition value AND gradient w.r.t. the candidates for one hyper-parameter sample (MAP): the EI x feasibility
// chain rule runs on the device right behind the moment gradients of the P outputs.
extern "C" int boss_acq_ei_grad(int P, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best,
                                double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    return acq_ei_grad_set_impl(P, 1, gps, M, Xs, mean_Xs, mean_grad, fit_coefs, y_max, has_best, best, valid_mask, acq_out, dacq_out, nullptr);
}

extern "C" int boss_acq_ei_grad_set(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                    const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best,
                                    double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    return acq_ei_grad_set_impl(P, S, gps, M, Xs, mean_Xs, mean_grad, fit_coefs, y_max, has_best, best, valid_mask, acq_out, dacq_out, nullptr);
}

// ------------------------------------------------------------------------------------------
// mean_and_var of a list of nonstationary posteriors at the same M candidates (boss_ngp_predict_set: the posteriors of the S samples
// of a Bayesian-inference fit, src/posterior.jl:15-19, each with its own latent models), boss_ngp_predict_grad over such a list
// (boss_ngp_predict_grad_set), and boss_acq_ei_grad_set's counterpart for them (boss_ngp_acq_ei_grad_set): one enqueue path.
// Candidates, every member's λ(x*), α(x*) and Jacobians go up once: lam_Xs d×M×n, amp_Xs M×n, mean_Xs null or M×n (member after
// member); equally shaped members (those of a boss_ngp_fit_batch) take the set launches, any other list goes member by member
// into the same slices (members_enqueue); one copy back.  The prediction calls clip the variances as boss_ngp_predict clips them:
// the first member with a variance below the threshold fails the call with BOSS_E_NEG_VAR, bad_index_out = the candidate.
// ------------------------------------------------------------------------------------------
struct NgpEiArgs {
    int P, S;
    const double *fit_coefs, *y_max;
    int has_best;
    double best;
    const unsigned char* valid_mask;
    double *acq_out, *dacq_out;
};

// ei: null (the members' moments come back: mu / var [n][M], and with dmu their gradients dmu / dvar [n][d×M]; dmu null: values
// only — no Jacobian, gradient or sum areas are reserved, and a handle whose update is still pending is refused as unfitted, which
// the gradient calls accept) or the acquisition's arguments (acq_out / dacq_out come back)
// lats: n resident latent objects (the _lat calls) instead of the four host arrays — the latent kernel fills the same buffers
static int ngp_grad_set_call(int n, boss_gp_t* const* gps, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                             const double* dlam_Xs, const double* damp_Xs, boss_nlat_t* const* lats, const double* mean_Xs, const double* mean_grad,
                             const NgpEiArgs* ei, double* mu, double* var, double* dmu, double* dvar, long* bad_index_out) {
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if ((long long)n * M > (1LL << 30)) return fail(BOSS_E_INVALID, "n·M above 2^30 is not supported");
    if (bad_index_out) *bad_index_out = -1;
    for (int i = 0; i < n; ++i) {
        if (!gps[i]) return fail(BOSS_E_INVALID, "NULL posterior handle");
        if (!gps[i]->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create / boss_ngp_fit_batch");
        if (gps[i]->ctx != gps[0]->ctx || gps[i]->d != gps[0]->d) return fail(BOSS_E_INVALID, "all handles must live on one device and share x_dim");
        if (gps[i]->discrete != gps[0]->discrete) return fail(BOSS_E_INVALID, "all handles must round the same dimensions");
    }
    boss_gp* g0 = gps[0];
    const int d = g0->d, Mp = round_up(M, 64);
    const bool grad = ei || dmu, accept_pending = grad;
    if (grad && d > GIBBS_GRAD_MAX_D) return fail(BOSS_E_INVALID, "x_dim above 16 is not supported by the nonstationary gradient kernel");
    if (grad && (long long)n * M * d * d > NGP_GRAD_SET_MAX_JAC) return fail(BOSS_E_INVALID, "n·M·x_dim² above 2^27 is not supported");
    for (int i = 0; i < n; ++i)
        if (!gps[i]->fitted && !(accept_pending && gps[i]->pending)) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    std::vector<NgpCand> pk(lats ? 1 : n);
    if (lats) {
        int rc = nlat_match(n, gps, lats);
        if (rc) return rc;
        ngp_pack_x(g0, M, Xs, pk[0]);
    }
    for (int i = 0; i < n && !lats; ++i) {
        int rc = ngp_pack(g0, M, Xs, lam_Xs + (size_t)i * d * M, amp_Xs + (size_t)i * M, pk[i]);
        if (rc) return rc;
    }
    Ctx* c = g0->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    for (int i = 0; i < n; ++i) {
        int rc = gp_settle(gps[i]);
        if (rc) return rc;
    }
    const size_t dm = (size_t)d * M, nm = (size_t)n * M, ndm = grad ? (size_t)n * dm : 0, nsums = grad ? (size_t)2 * (2 * d + 1) * Mp : 0;
    const int P = ei ? ei->P : 0;
    const bool has_jl = grad && (lats || dlam_Xs), has_ja = grad && (lats || damp_Xs);
    // candidates | λ(x*) of every member | α(x*) of every member | ∂λ/∂x | ∂α/∂x [| the latent kernel's flag]
    int rc = ws_reserve(c->craw, sizeof(double) * ((size_t)d * Mp + (size_t)n * ((size_t)d * Mp + Mp) + (has_jl ? ndm * d : 0) + (has_ja ? ndm : 0) + (lats ? 1 : 0)));
    if (rc) return rc;
    // acq | dacq | mu | var | dmu | dvar | bad | mean | mean_grad | sums of one member (member-by-member path) | coefs | ymax | mask
    const size_t nacq = ei ? M + dm : 0, nd = nacq + 3 * nm + 3 * ndm + 1 + nsums + 2 * (size_t)P;
    rc = ws_reserve(c->pred, sizeof(double) * nd + (ei ? M : 0));
    if (rc) return rc;
    boss_cand cd;
    cd.ctx = c;
    cd.d = d;
    cd.M = M;
    cd.Mp = Mp;
    cd.Craw = (double*)c->craw.p;
    double* clam = cd.Craw + (size_t)d * Mp;
    double* camp = clam + (size_t)n * d * Mp;
    double* djl = camp + (size_t)n * Mp;
    double* dja = djl + (has_jl ? ndm * d : 0);
    double* dacq = (double*)c->pred.p;
    double* ddacq = dacq + (ei ? M : 0);
    double* dmu_ = dacq + nacq;
    double* dvar_ = dmu_ + nm;
    double* dgm = dvar_ + nm;
    double* dgv = dgm + ndm;
    unsigned long long* dbad = (unsigned long long*)(dgv + ndm);
    double* dmean = dgv + ndm + 1;
    double* dmg = dmean + nm;
    double* dsums = dmg + ndm;
    double* dcoef = dsums + nsums;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(dacq + nd);
    EiPar par;
    if (ei) {
        rc = ei_params(c, s, P, ei->fit_coefs, ei->y_max, ei->has_best, ei->best, &par, dcoef, dymax);
        if (rc) return drain(c, rc);
    }
    HIPCHK(hipMemcpyAsync(cd.Craw, pk[0].x.data(), sizeof(double) * d * Mp, hipMemcpyHostToDevice, s));
    for (int i = 0; i < n && !lats; ++i) {
        HIPCHK(hipMemcpyAsync(clam + (size_t)i * d * Mp, pk[i].lam.data(), sizeof(double) * d * Mp, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(camp + (size_t)i * Mp, pk[i].amp.data(), sizeof(double) * Mp, hipMemcpyHostToDevice, s));
    }
    if (dlam_Xs) HIPCHK(hipMemcpyAsync(djl, dlam_Xs, sizeof(double) * ndm * d, hipMemcpyHostToDevice, s));
    if (damp_Xs) HIPCHK(hipMemcpyAsync(dja, damp_Xs, sizeof(double) * ndm, hipMemcpyHostToDevice, s));
    if (lats) {
        unsigned long long* lbad = (unsigned long long*)(dja + ndm);
        rc = nlat_enqueue(c, n, lats, cd.Craw, Mp, M, clam, (size_t)d * Mp, camp, (size_t)Mp, grad ? djl : nullptr, grad ? dm * d : 0,
                          grad ? dja : nullptr, grad ? dm : 0, nullptr, lbad);
        if (rc == BOSS_OK) rc = nlat_check(c, lbad, nullptr);
        if (rc) return drain(c, rc);
    }
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * nm, hipMemcpyHostToDevice, s);
    if (mean_grad && grad) (void)hipMemcpyAsync(dmg, mean_grad, sizeof(double) * ndm, hipMemcpyHostToDevice, s);
    if (ei && ei->valid_mask) (void)hipMemcpyAsync(dmask, ei->valid_mask, M, hipMemcpyHostToDevice, s);
    if (!ei) (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
    if (!ei || par.mode != 0) {
        MemberSlices q;
        q.mean = mean_Xs ? dmean : nullptr;
        q.mean_grad = mean_grad && grad ? dmg : nullptr;
        q.mu = dmu_, q.var = dvar_, q.gm = grad ? dgm : nullptr, q.gv = grad ? dgv : nullptr;
        q.clam = clam, q.camp = camp, q.dlam = has_jl ? djl : nullptr, q.damp = has_ja ? dja : nullptr;
        q.sums = dsums;
        rc = members_enqueue(n, gps, &cd, q, true);
        if (rc) return drain(c, rc);
    }
    if (ei) {
        // (ei_grad_set_kernel for every S, 1 included)
        ei_grad_epilogue_launch(s, dmu_, dvar_, dgm, dgv, M, d, ei->S, false, par, dcoef, dymax, ei->valid_mask ? dmask : nullptr, nullptr, nullptr,
                                dacq, ddacq);
        return finish(c, {{ei->acq_out, dacq, sizeof(double) * M}, {ei->dacq_out, ddacq, sizeof(double) * dm}});
    }
    // (member after member in one array: the smallest flat index is the first member's first offender)
    hipLaunchKernelGGL(clip_var_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, dvar_, (int)nm, dbad);
    unsigned long long bad = 0;
    if (grad)
        rc = finish(c, {{mu, dmu_, sizeof(double) * nm}, {var, dvar_, sizeof(double) * nm}, {dmu, dgm, sizeof(double) * ndm},
                        {dvar, dgv, sizeof(double) * ndm}, {&bad, dbad, sizeof bad}});
    else
        rc = finish(c, {{mu, dmu_, sizeof(double) * nm}, {var, dvar_, sizeof(double) * nm}, {&bad, dbad, sizeof bad}});
    if (rc) return rc;
    return bad != ~0ULL ? neg_var_error(bad_index_out, bad % (unsigned long long)M, var[bad]) : BOSS_OK;
}

extern "C" int boss_ngp_predict_set(int n, boss_gp_t* const* gps, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                                    const double* mean_Xs, double* mu, double* var, long* bad_index_out) {
    if (n < 1 || !gps || !Xs || !lam_Xs || !amp_Xs || !mu || !var) return fail(BOSS_E_INVALID, "NULL argument or n < 1");
    return ngp_grad_set_call(n, gps, M, Xs, lam_Xs, amp_Xs, nullptr, nullptr, nullptr, mean_Xs, nullptr, nullptr, mu, var, nullptr, nullptr, bad_index_out);
}
extern "C" int boss_ngp_predict_set_lat(int n, boss_gp_t* const* gps, int M, const double* Xs, boss_nlat_t* const* lats,
                                        const double* mean_Xs, double* mu, double* var, long* bad_index_out) {
    if (n < 1 || !gps || !Xs || !lats || !mu || !var) return fail(BOSS_E_INVALID, "NULL argument or n < 1");
    return ngp_grad_set_call(n, gps, M, Xs, nullptr, nullptr, nullptr, nullptr, lats, mean_Xs, nullptr, nullptr, mu, var, nullptr, nullptr, bad_index_out);
}
extern "C" int boss_ngp_predict_grad_set(int n, boss_gp_t* const* gps, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                                         const double* dlam_Xs, const double* damp_Xs, const double* mean_Xs, const double* mean_grad,
                                         double* mu, double* var, double* dmu, double* dvar, long* bad_index_out) {
    if (n < 1 || !gps || !Xs || !lam_Xs || !amp_Xs || !mu || !var || !dmu || !dvar) return fail(BOSS_E_INVALID, "NULL argument or n < 1");
    return ngp_grad_set_call(n, gps, M, Xs, lam_Xs, amp_Xs, dlam_Xs, damp_Xs, nullptr, mean_Xs, mean_grad, nullptr, mu, var, dmu, dvar, bad_index_out);
}
extern "C" int boss_ngp_predict_grad_set_lat(int n, boss_gp_t* const* gps, int M, const double* Xs, boss_nlat_t* const* lats,
                                             const double* mean_Xs, const double* mean_grad, double* mu, double* var, double* dmu,
                                             double* dvar, long* bad_index_out) {
    if (n < 1 || !gps || !Xs || !lats || !mu || !var || !dmu || !dvar) return fail(BOSS_E_INVALID, "NULL argument or n < 1");
    return ngp_grad_set_call(n, gps, M, Xs, nullptr, nullptr, nullptr, nullptr, lats, mean_Xs, mean_grad, nullptr, mu, var, dmu, dvar, bad_index_out);
}

// The acquisition of boss_acq_ei_grad_set for nonstationary posteriors: gps[p + P·s], every member with its own latent values and
// Jacobians at the candidates; per sample the chain rule of boss_acq_ei_grad_moments on its P members' moments and gradients, the
// samples summed in ascending s and divided once (ei_grad_set_kernel).  Nothing but acq / dacq leaves the device.
extern "C" int boss_ngp_acq_ei_grad_set(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* lam_Xs,
                                        const double* amp_Xs, const double* dlam_Xs, const double* damp_Xs, const double* mean_Xs,
                                        const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best, double best,
                                        const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    if (P < 1 || S < 1 || !gps || !Xs || !lam_Xs || !amp_Xs || !fit_coefs || !acq_out || !dacq_out) return fail(BOSS_E_INVALID, "bad arguments");
    if ((long long)P * S > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M above 2^30 is not supported");
    const NgpEiArgs ei{P, S, fit_coefs, y_max, has_best, best, valid_mask, acq_out, dacq_out};
    return ngp_grad_set_call(P * S, gps, M, Xs, lam_Xs, amp_Xs, dlam_Xs, damp_Xs, nullptr, mean_Xs, mean_grad, &ei, nullptr, nullptr, nullptr, nullptr,
                             nullptr);
}
extern "C" int boss_ngp_acq_ei_grad_set_lat(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, boss_nlat_t* const* lats,
                                            const double* mean_Xs, const double* mean_grad, const double* fit_coefs, const double* y_max,
                                            int has_best, double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    if (P < 1 || S < 1 || !gps || !Xs || !lats || !fit_coefs || !acq_out || !dacq_out) return fail(BOSS_E_INVALID, "bad arguments");
    if ((long long)P * S > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M above 2^30 is not supported");
    const NgpEiArgs ei{P, S, fit_coefs, y_max, has_best, best, valid_mask, acq_out, dacq_out};
    return ngp_grad_set_call(P * S, gps, M, Xs, nullptr, nullptr, nullptr, nullptr, lats, mean_Xs, mean_grad, &ei, nullptr, nullptr, nullptr, nullptr,
                             nullptr);
}

// The same chain rule from moments and moment gradients the caller already holds (nonstationary posteriors: boss_ngp_predict_grad per
// output; outputs fitted on other ranks): mu / var [p][M] (var clipped), dmu / dvar [p][d×M column-major per candidate].
extern "C" int boss_acq_ei_grad_moments(int device, int P, int M, int d, const double* mu, const double* var, const double* dmu,
                                        const double* dvar, const double* fit_coefs, const double* y_max, int has_best, double best,
                                        const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    if (P < 1 || M < 1 || d < 1 || !mu || !var || !dmu || !dvar || !fit_coefs || !acq_out || !dacq_out) return fail(BOSS_E_INVALID, "bad arguments");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const size_t dm = (size_t)d * M;
    const size_t nd = (size_t)2 * P * M + (size_t)2 * P * dm + M + dm + 2 * P;
    rc = ws_reserve(c->pred, sizeof(double) * nd + M);
    if (rc) return rc;
    double* dev = (double*)c->pred.p;
    double* d_mu = dev;
    double* d_var = d_mu + (size_t)P * M;
    double* d_gm = d_var + (size_t)P * M;
    double* d_gv = d_gm + (size_t)P * dm;
    double* dacq = d_gv + (size_t)P * dm;
    double* ddacq = dacq + M;
    double* dcoef = ddacq + dm;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(dev + nd);
    EiPar par;
    rc = ei_params(c, s, P, fit_coefs, y_max, has_best, best, &par, dcoef, dymax);
    if (rc) return drain(c, rc);
    (void)hipMemcpyAsync(d_mu, mu, sizeof(double) * P * M, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_var, var, sizeof(double) * P * M, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_gm, dmu, sizeof(double) * P * dm, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_gv, dvar, sizeof(double) * P * dm, hipMemcpyHostToDevice, s);
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    ei_grad_epilogue_launch(s, d_mu, d_var, d_gm, d_gv, M, d, 1, true, par, dcoef, dymax, valid_mask ? dmask : nullptr, nullptr, nullptr, dacq, ddacq);
    return finish(c, {{acq_out, dacq, sizeof(double) * M}, {dacq_out, ddacq, sizeof(double) * dm}});
}

// ------------------------------------------------------------------------------------------
// mean_and_cov / cov: V = L⁻¹K* from predict_enqueue(need_v), then Σ = K** − VᵀV.  Gradient-observation and nonstationary
// posteriors: VᵀV on the fp64 MFMA in 64×64 lower-triangle block pairs × chunks of the n range (cov_syrk_partial_kernel) and the
// fixed-order sum with K** (cov_finish_kernel).  Plain posteriors: the VALU predict_cov_kernel + clip_cov_diag_kernel.
// ------------------------------------------------------------------------------------------
constexpr int COV_MAX_M = 32768;                // M×M doubles = 8 GiB on the device and on the host
constexpr int COV_TARGET_WG = 512;              // (block pair, chunk) workgroups wanted: two per CU
constexpr size_t COV_PART_MIN_CAP = 64ull << 20;

// Block pairs P, chunks C of `rows` training rows each.  The partial slabs (C·P blocks of 64×64 doubles) are bounded by the larger
// of the M×M output and 64 MiB: small M gets up to Np/256 chunks (M = 64: 3 block pairs), large M one chunk (P·32 KiB ≈ 4 M² bytes).
static void cov_plan(int Np, int M, int& P, int& C, int& rows) {
    const int nbk = (M + COV_T - 1) / COV_T;
    P = nbk * (nbk + 1) / 2;
    const int nrb = Np / PRED_RB;
    const size_t slab = (size_t)P * COV_T * COV_T * sizeof(double);
    const size_t cap = std::max((size_t)M * M * sizeof(double), COV_PART_MIN_CAP);
    int want = (COV_TARGET_WG + P - 1) / P;
    want = (int)std::min<size_t>((size_t)want, std::max<size_t>(1, cap / slab));
    want = std::max(1, std::min(want, nrb));
    const int per = (nrb + want - 1) / want;              // 256-row blocks per chunk
    rows = per * PRED_RB;
    C = (nrb + per - 1) / per;
}

// enqueue Σ into dcov (M×M) from the V slabs predict_enqueue(need_v = true) just left; part has room for cov_plan's C·P blocks
static void cov_enqueue(boss_gp* g, int M, int form, const double* X, const double* Lam, const double* Amp, int ldx, double* part,
                        double* dcov, unsigned long long* dbad) {
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    int P, C, rows;
    cov_plan(g->Np, M, P, C, rows);
    ProfScope ps(c, "cov");
    hipLaunchKernelGGL(cov_syrk_partial_kernel, dim3(P, C), dim3(256), 0, s, (const double*)c->vscratch.p, g->Np, slab_bn(M, false), M,
                       rows, part);
    if (form == COV_FORM_GIBBS)
        hipLaunchKernelGGL(cov_finish_kernel<COV_FORM_GIBBS>, dim3(P), dim3(256), 0, s, (const double*)part, C, X, Lam, Amp, g->d, ldx,
                           g->kernel, g->amp2, M, dcov, dbad);
    else
        hipLaunchKernelGGL(cov_finish_kernel<COV_FORM_VALUE>, dim3(P), dim3(256), 0, s, (const double*)part, C, X, Lam, Amp, g->d, ldx,
                           g->kernel, g->amp2, M, dcov, dbad);
}

static size_t cov_part_doubles(const boss_gp* g, int M) {
    int P, C, rows;
    cov_plan(g->Np, M, P, C, rows);
    return (size_t)C * P * COV_T * COV_T;
}

// The three covariance entry points behind their argument checks: candidates staged (pk: packed by ngp_pack, else Xs through
// temp_cand), μ and V, Σ, copied back, the clipping error of Σ's diagonal (none for gradient observations: their Σ is not clipped).
// Σ and the partial slabs are a per-call allocation: up to 8 GiB must not stay resident in a grow-only workspace.
static int predict_cov(boss_gp* g, int M, const double* Xs, const NgpCand* pk, const double* mean_Xs, double* mu, double* cov,
                       long* bad_index) {
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);                 // the V slabs live in the shared scratch
    hipStream_t s = c->stream;
    boss_cand cd;
    double *clam = nullptr, *camp = nullptr;
    int rc = pk ? ngp_upload(c, g->d, M, *pk, cd, clam, camp) : temp_cand(c, g->d, M, Xs, &cd);
    if (rc) return drain(c, rc);
    const size_t MM = (size_t)M * M;
    double* dev = nullptr;   // mu | cov | bad | var | mean | partials
    if (dev_malloc((void**)&dev, sizeof(double) * (3 * (size_t)M + 2 + MM + (g->aug || g->gibbs ? cov_part_doubles(g, M) : 0))) != hipSuccess)
        return drain(c, fail(BOSS_E_ALLOC, "device allocation failed"));
    double *dmu = dev, *dcov = dev + M, *dvar = dcov + MM + 1, *dmean = dvar + M, *part = dmean + M;
    unsigned long long* dbad = g->aug ? nullptr : (unsigned long long*)(dcov + MM);
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s);
    if (dbad) (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
    rc = predict_enqueue(g, &cd, mean_Xs ? dmean : nullptr, dmu, dvar, false, clam, camp, true);   // V in the slab scratch, Csc scaled
    if (rc) {
        (void)drain(c, rc);
        (void)hipFree(dev);
        return rc;
    }
    if (g->gibbs) {
        cov_enqueue(g, M, COV_FORM_GIBBS, (const double*)cd.Craw, clam, camp, cd.Mp, part, dcov, dbad);
    } else if (g->aug) {
        cov_enqueue(g, M, COV_FORM_VALUE, (const double*)c->csc.p, nullptr, nullptr, cd.Mp, part, dcov, nullptr);
    } else {
        const int gb = (M + 15) / 16;
        hipLaunchKernelGGL(predict_cov_kernel, dim3(gb, gb), dim3(256), 0, s, (const double*)c->vscratch.p, g->Np, slab_bn(M, false),
                           (const double*)c->csc.p, g->d, cd.Mp, M, g->kernel, g->amp2, dcov);
        hipLaunchKernelGGL(clip_cov_diag_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dcov, M, dbad);
    }
    unsigned long long bad = ~0ULL;
    rc = dbad ? finish(c, {{mu, dmu, sizeof(double) * M}, {cov, dcov, sizeof(double) * MM}, {&bad, dbad, sizeof bad}})
              : finish(c, {{mu, dmu, sizeof(double) * M}, {cov, dcov, sizeof(double) * MM}});
    (void)hipFree(dev);
    if (rc) return rc;
    return bad != ~0ULL ? neg_var_error(bad_index, bad, cov[bad * (size_t)M + bad]) : BOSS_OK;
}

extern "C" int boss_gp_predict_cov(boss_gp_t* g, int M, const double* Xs, const double* mean_Xs, double* mu,
                                   double* cov, long* bad_index) {
    if (!g || !Xs || !mu || !cov) return fail(BOSS_E_INVALID, "NULL argument");
    NOT_FOR_AUG(g);
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (bad_index) *bad_index = -1;
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    return predict_cov(g, M, Xs, nullptr, mean_Xs, mu, cov, bad_index);
}

extern "C" int boss_ggp_predict_cov(boss_gp_t* g, int M, const double* Xs, double* mu, double* cov) {
    if (!g || !Xs || !mu || !cov) return fail(BOSS_E_INVALID, "NULL argument");
    if (!g->aug) return fail(BOSS_E_INVALID, "handle was not created by boss_ggp_create");
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (M > COV_MAX_M) return fail(BOSS_E_INVALID, "M above the covariance limit of 32768 candidates");
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    return predict_cov(g, M, Xs, nullptr, nullptr, mu, cov, nullptr);
}

extern "C" int boss_ngp_predict_cov(boss_gp_t* g, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                                    const double* mean_Xs, double* mu, double* cov, long* bad_index) {
    if (!g || !Xs || !lam_Xs || !amp_Xs || !mu || !cov) return fail(BOSS_E_INVALID, "NULL argument");
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (M > COV_MAX_M) return fail(BOSS_E_INVALID, "M above the covariance limit of 32768 candidates");
    if (bad_index) *bad_index = -1;
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    NgpCand pk;
    int rc = ngp_pack(g, M, Xs, lam_Xs, amp_Xs, pk);
    if (rc) return rc;
    return predict_cov(g, M, Xs, &pk, mean_Xs, mu, cov, bad_index);
}
