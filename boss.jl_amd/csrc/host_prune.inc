// host_prune.inc — the arg-max-only acquisition path (kernels: prune_kernels.hpp; included by bosship.hip before host_acq.inc).
//
// boss_acq_ei without acq_out returns the arg-max and its value only.  EI is non-decreasing in σ and in c·μ − best, the exact mean
// needs no substitution (μ = m + k*ᵀa, a = L⁻ᵀz), and the variance after the first s 256-row blocks of the substitution bounds the
// final one from above: EI(μ, σ²_s) is an upper bound on a candidate's EI at s(s+1)/2 of the fused kernel's block products.  The K
// largest bounds are finished exactly (round 1, the few-candidates path), their maximum T prunes every candidate with ub < T, and
// what is left (round 2) is finished the same way.  A pruned candidate has EI <= ub < T <= max: it can neither win nor tie.

struct PruneCfg {
    int min_tiles = -1;        // candidate tiles above which the path is tried (-1: the few-candidates limit)
    int K = 64;                // round-1 size
    int s = 1;                 // 256-row blocks of the head variance (measured at N = 4096, M = 8192: 0.83 / 0.87 / 0.98 ms for 1 / 2 / 4)
    int cap = 1024;            // round-2 size beyond which the full kernel runs
    double slack = 1.0;        // scale of the slacks (tests: 0)
};
static PruneCfg g_prune;
// slacks of the bound (DESIGN.md §4.5): δμ = PRUNE_KMU (|c μ| + |best| + |c| α), δv = PRUNE_KVAR α².  100 × the largest relative
// |μ_a − μ| seen on the device over the hyper-parameter grid of tests/regimes_cases.py (1.13e-6: sqexp, λ_rel 30, α 30, σ 1e-3);
// σ²_fused − σ²_s was never positive there, its slack is 100 × rows·2⁻⁵³ at 9000 rows
constexpr double PRUNE_KMU = 1.2e-4, PRUNE_KVAR = 1e-10;
constexpr size_t PRUNE_RES_OFF = 16;   // doubles into the pinned result block: {max, index, count, flag, sequence}

static bool prune_enabled() {
    static const bool on = !(getenv("BOSS_ACQ_PRUNE") && atoi(getenv("BOSS_ACQ_PRUNE")) == 0);
    static const bool once = [] {
        if (getenv("BOSS_ACQ_PRUNE_BLOCKS")) g_prune.s = std::max(1, atoi(getenv("BOSS_ACQ_PRUNE_BLOCKS")));
        if (getenv("BOSS_ACQ_PRUNE_CAP")) g_prune.cap = std::max(0, atoi(getenv("BOSS_ACQ_PRUNE_CAP")));
        return true;
    }();
    (void)once;
    return on;
}

extern "C" int boss_debug_acq_path(int device, int* out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mtx);
    for (int i = 0; i < 5; ++i) out[i] = c->prune_last[i];
    return BOSS_OK;
}
// tests: reach the path at small sizes (an argument of -1 keeps the current value, anything below restores the default)
extern "C" int boss_debug_acq_prune_set(int device, int min_tiles, int K, int s, int cap) {
    (void)device;
    (void)prune_enabled();                                   // (the environment is read first: it does not override this call later)
    const PruneCfg def;
    if (min_tiles != -1) g_prune.min_tiles = min_tiles < -1 ? def.min_tiles : min_tiles;
    if (K != -1) g_prune.K = K < 1 ? def.K : K;
    if (s != -1) g_prune.s = s < 1 ? def.s : s;
    if (cap != -1) g_prune.cap = cap < -1 ? def.cap : cap;
    return BOSS_OK;
}
// tests: {the handle's resident inverse factors exist, its few-candidates call count, device allocations of the process, kernels the
// pruned path enqueued on the handle's device} — a repeated arg-max-only call must change none of the first three
extern "C" int boss_debug_acq_counters(const boss_gp* g, long* out) {
    if (!g || !out) return fail(BOSS_E_INVALID, "NULL argument");
    out[0] = g->have_winv ? 1 : 0;
    out[1] = g->few_calls;
    out[2] = g_dev_allocs.load();
    out[3] = g->ctx->prune_launches;
    return BOSS_OK;
}
extern "C" int boss_debug_acq_prune_slack(int device, double scale) {
    (void)device;
    if (!(scale >= 0.0)) return fail(BOSS_E_INVALID, "scale must be >= 0");
    g_prune.slack = scale;
    return BOSS_OK;
}
// measurements: μ_a, σ²_s and the bounds the last pruned attempt on the device left (M doubles each, any may be NULL)
extern "C" int boss_debug_acq_prune_bounds(int device, int M, double* mua_out, double* vars_out, double* ub_out) {
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mtx);
    if (M < 1 || M != c->prune_M || !c->prunews.p) return fail(BOSS_E_INVALID, "no pruned attempt with that many candidates");
    HIPCHK(hipStreamSynchronize(c->stream));
    const double* base = (const double*)c->prunews.p;
    if (mua_out) HIPCHK(hipMemcpy(mua_out, base, sizeof(double) * M, hipMemcpyDeviceToHost));
    if (vars_out) HIPCHK(hipMemcpy(vars_out, base + M, sizeof(double) * M, hipMemcpyDeviceToHost));
    if (ub_out) HIPCHK(hipMemcpy(ub_out, base + 2 * (size_t)M, sizeof(double) * M, hipMemcpyDeviceToHost));
    return BOSS_OK;
}

// may this call take the pruned path?  (everything else keeps the full kernel: see the conditions in DESIGN.md §4.5)
static bool prune_eligible(const boss_gp* g, const boss_cand* cd, int P, int S, const EiPar& par, bool has_out, bool defer, bool has_mc,
                           const double* dpair) {
    if (!prune_enabled() || has_out || defer || dpair || has_mc || P != 1 || S != 1 || par.mode != 1) return false;
    if (g->aug || g->gibbs || g->kprog || g->ctx->prof_on) return false;
    const int ftiles = (cd->M + 31) / 32;                    // (few_max_tiles: predict_enqueue's limit of its few-candidates branch — the rounds must stay below it)
    const int min_tiles = g_prune.min_tiles >= 0 ? g_prune.min_tiles : few_max_tiles();
    if (few_off() || ftiles <= min_tiles || g->Np < 4 * PRED_RB || g->d > 64 || cd->d != g->d || slab_bn(cd->M, false) != 32) return false;
    if (small_predict_ok(g, cd->M) || cd->M <= g_prune.K || cd->M > PRUNE_THREADS * PRUNE_CPT_MAX) return false;
    if (g_prune.K > 32 * few_max_tiles()) return false;       // (round 1 would not reach the few-candidates branch)
    return g_prune.s < g->Np / PRED_RB;
}

static bool prune_poll(Ctx* c, hipStream_t s, const double* res, unsigned long long want) {
    volatile const unsigned long long* seq = reinterpret_cast<volatile const unsigned long long*>(res) + 4;
    bool got = false;
    for (unsigned long i = 1;; ++i) {
        if (*seq == want) {
            got = true;
            break;
        }
        if ((i & 0x3fff) == 0 && hipStreamQuery(s) != hipErrorNotReady) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!got) {
        (void)hipStreamSynchronize(s);
        got = *seq == want;
    }
    return got;
}

// a = L⁻ᵀz current on the stream for this factorisation: the gradient path's vector when it is, else the handle's own, rebuilt by
// one launch per 256-row step.  *rebuilt reports whether the chain ran.
static int prune_avec(boss_gp* g, hipStream_t s, const double** a_out, bool* rebuilt) {
    *rebuilt = false;
    if (g->have_lt && g->avec) {
        *a_out = g->avec;
        return BOSS_OK;
    }
    if (g->prune_a && g->prune_a_np != g->Np) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(g->prune_a);
        g->prune_a = nullptr;
    }
    if (!g->prune_a) {
        if (dev_malloc((void**)&g->prune_a, sizeof(double) * 2 * (size_t)g->Np) != hipSuccess) {
            g->prune_a = nullptr;
            return fail(BOSS_E_ALLOC, "device allocation failed");
        }
        g->prune_a_np = g->Np;
        g->prune_a_gen = ~0ull;
    }
    if (g->prune_a_gen != g->factor_gen) {
        const int nb = g->Np / PRED_RB;
        for (int ib = nb - 1; ib >= 0; --ib)
            hipLaunchKernelGGL(prune_avec_step_kernel, dim3(std::max(1, 2 * ib)), dim3(PRUNE_AVEC_THREADS), 0, s, (const double*)g->A, g->ld, g->Np, g->N,
                               (const double*)g->Dinv2, ib, ib == nb - 1 ? 1 : 0, g->prune_a + g->Np, g->prune_a);
        g->prune_a_gen = g->factor_gen;
        *rebuilt = true;
    }
    *a_out = g->prune_a;
    return BOSS_OK;
}

// Returns BOSS_OK with *done = true and (max, arg-max) in res_out / idx_out when the pruned path answered; *done = false: the caller
// runs the full kernel (nothing it relies on was touched beyond the scaled candidates, which it writes again).
static int acq_prune_try(boss_gp* g, const boss_cand* cd, const double* mean_dev, const unsigned char* mask_dev, const EiPar& par,
                         bool* done, double* res_out, long* idx_out) {
    *done = false;
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    int* last = c->prune_last;
    last[0] = 0;
    last[1] = last[2] = last[4] = 0;
    last[3] = g_prune.s;
    if (g->prune_skip > 0) {
        --g->prune_skip;
        last[0] = 3;
        return BOSS_OK;
    }
    const int M = cd->M, Mp = cd->Mp, d = g->d, Np = g->Np, nch = Np / PRUNE_MU_ROWS, sblk = g_prune.s, K = g_prune.K;
    // (a round 2 beyond the few-candidates limit would run the fused kernel on the internal block: the full kernel answers instead)
    const int cap = std::min(g_prune.cap, 32 * few_max_tiles()), tiles = (M + 31) / 32;
    const size_t nint = (size_t)round_up(std::max(K, cap), 64);            // columns of the internal candidate block
    // doubles: μ_a | σ²_s | ub | keys | part [nch][M] | μ, σ², m of the internal block | its coordinates [d][nint] | (T, index)
    const size_t nd = (size_t)4 * M + (size_t)nch * M + 3 * nint + (size_t)d * nint + 2;
    int rc = ws_reserve(c->prunews, sizeof(double) * nd + sizeof(int) * (nint + (size_t)M) + (size_t)M);
    if (rc) return rc;
    rc = ws_reserve(c->csc, sizeof(double) * (size_t)d * Mp);
    if (rc) return rc;
    rc = ws_reserve(c->vscratch, sizeof(double) * (size_t)tiles * 32 * Np);   // (what the full kernel reserves: a fallback allocates nothing)
    if (rc) return rc;
    double* mua = (double*)c->prunews.p;
    double* vars = mua + M;
    double* ub = vars + M;
    unsigned long long* keys = (unsigned long long*)(ub + M);
    double* part = ub + 2 * (size_t)M;
    double* imu = part + (size_t)nch * M;
    double* ivar = imu + nint;
    double* imean = ivar + nint;
    double* icraw = imean + nint;
    double* tpair = icraw + (size_t)d * nint;
    int* sel = (int*)(tpair + 2);
    int* surv = sel + nint;
    unsigned char* insel = (unsigned char*)(surv + M);
    c->prune_M = M;
    double* res = (double*)c->pinned + PRUNE_RES_OFF;

    if (!g->have_dinv) {
        dinv_join(g);
        dinv_launch(g, s);
        g->have_dinv = true;
    }
    dinv_join(g);
    g->dinv_used = true;
    const double* avec = nullptr;
    bool rebuilt = false;
    rc = prune_avec(g, s, &avec, &rebuilt);
    if (rc) return rc;
    last[4] = rebuilt ? 1 : 0;
    c->prune_launches += (rebuilt ? Np / PRED_RB : 0) + 7;   // chain, then scaling, head, means, bounds, selection, gather, decision
    double* Csc = (double*)c->csc.p;
    hipLaunchKernelGGL(scale_cand_kernel, dim3((Mp + 255) / 256), dim3(256), 0, s, cd->Craw, Csc, g->invlam, g->discrete_dev, d, Mp);
    typedef PredG32 G;
    hipLaunchKernelGGL(prune_head_kernel<G>, dim3(tiles), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, (const double*)g->A, g->ld, Np, g->N,
                       (const double*)g->Dinv2, (const double*)g->Xsc, (const double*)Csc, d, Mp, g->kernel, g->amp2, (double*)c->vscratch.p, M,
                       sblk, vars);
    const size_t mu_lds = sizeof(double) * ((size_t)d + 1) * PRUNE_MU_STAGE;
    auto mu_fn = d <= 16 ? prune_mu_kernel<true> : prune_mu_kernel<false>;
    hipLaunchKernelGGL(mu_fn, dim3((M + PRUNE_MU_CANDS - 1) / PRUNE_MU_CANDS, nch), dim3(256), mu_lds, s, (const double*)g->Xsc, Np, g->N, (const double*)Csc, d, Mp, M,
                       g->kernel, g->amp2, avec, part);
    PrunePar pp;
    pp.coef = par.coefs[0];
    pp.best = par.best;
    pp.amp2 = g->amp2;
    pp.kmu = PRUNE_KMU * g_prune.slack;
    pp.kvar = PRUNE_KVAR * g_prune.slack;
    hipLaunchKernelGGL(prune_bound_kernel, dim3((M + 255) / 256), dim3(256), 0, s, (const double*)part, nch, mean_dev, (const double*)vars, mask_dev, M,
                       pp, mua, ub, keys);
    hipLaunchKernelGGL(prune_select_kernel, dim3(1), dim3(PRUNE_THREADS), 0, s, (const unsigned long long*)keys, M, K, sel, insel);

    // round 1: the K largest bounds, exactly, by the few-candidates path on an internal resident block
    boss_cand icd;
    icd.ctx = c;
    icd.d = d;
    auto finish_exact = [&](const int* list, int n) -> int {
        icd.M = n;
        icd.Mp = round_up(n, 64);
        icd.Craw = icraw;
        hipLaunchKernelGGL(prune_gather_kernel, dim3((icd.Mp + 255) / 256), dim3(256), 0, s, list, n, (const double*)cd->Craw, Mp, d, mean_dev,
                           icraw, icd.Mp, mean_dev ? imean : (double*)nullptr);
        return predict_enqueue(g, &icd, mean_dev ? imean : nullptr, imu, ivar, false, nullptr, nullptr, false, true);
    };
    rc = finish_exact(sel, K);
    if (rc) return drain(c, rc);
    unsigned long long seq = ++c->acq_seq;
    hipLaunchKernelGGL(prune_decide_kernel, dim3(1), dim3(PRUNE_THREADS), 0, s, (const int*)sel, K, (const double*)imu, (const double*)ivar,
                       (const double*)mua, mask_dev, par, pp, M, (const double*)ub, (const unsigned char*)insel, surv, tpair, res, seq);
    bool ok = prune_poll(c, s, res, seq);
    hipError_t e = hipGetLastError();
    if (!ok || e != hipSuccess) return fail(BOSS_E_NO_DEVICE, e != hipSuccess ? hipGetErrorString(e) : "the pruned acquisition did not report");
    long cnt = reinterpret_cast<const long*>(res)[2], bad = reinterpret_cast<const long*>(res)[3];
    last[1] = K;
    last[2] = (int)std::min<long>(cnt, 0x7fffffff);
    if (!bad && cnt > 0 && cnt <= cap) {
        rc = finish_exact(surv, (int)cnt);
        if (rc) return drain(c, rc);
        c->prune_launches += 2;
        seq = ++c->acq_seq;
        hipLaunchKernelGGL(prune_merge_kernel, dim3(1), dim3(PRUNE_THREADS), 0, s, (const int*)surv, (int)cnt, (const double*)imu,
                           (const double*)ivar, (const double*)mua, mask_dev, par, pp, (const double*)tpair, res, seq);
        ok = prune_poll(c, s, res, seq);
        e = hipGetLastError();
        if (!ok || e != hipSuccess) return fail(BOSS_E_NO_DEVICE, e != hipSuccess ? hipGetErrorString(e) : "the pruned acquisition did not report");
        bad = reinterpret_cast<const long*>(res)[3];
    }
    if (bad || cnt > cap) {
        // the mean check failed, or too many contenders: the full kernel answers, and the next attempts wait 1, 2, 4 … 64 calls
        g->prune_backoff = g->prune_backoff ? std::min(64, 2 * g->prune_backoff) : 1;
        g->prune_skip = g->prune_backoff;
        last[0] = 2;
        return BOSS_OK;
    }
    g->prune_backoff = 0;
    last[0] = 1;
    *res_out = res[0];
    *idx_out = reinterpret_cast<const long*>(res)[1];
    *done = true;
    return BOSS_OK;
}
