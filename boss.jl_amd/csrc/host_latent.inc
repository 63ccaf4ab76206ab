// host_latent.inc — resident latent models of a NonstationaryGP (boss_nlat_*; latent_kernels.hpp) and the staging step the _lat
// prediction calls of host_predict.inc share with them (included by bosship.hip).

// The transposed factor, the transposed 256×256 inverses and a = L⁻ᵀz = (K+σ²I)⁻¹(y−m) of a handle: storage ...
static int lt_alloc(boss_gp* g) {
    if (g->LT) return BOSS_OK;
    const int Np = g->Np;
    if (dev_malloc((void**)&g->LT, sizeof(double) * (size_t)g->ld * Np) != hipSuccess ||
        dev_malloc((void**)&g->DT2, sizeof(double) * (size_t)Np * PRED_RB) != hipSuccess ||
        dev_malloc((void**)&g->avec, sizeof(double) * (size_t)Np * 2) != hipSuccess) {
        if (g->LT) (void)hipFree(g->LT);
        if (g->DT2) (void)hipFree(g->DT2);
        g->LT = g->DT2 = g->avec = nullptr;
        (void)hipGetLastError();
        return fail(BOSS_E_ALLOC, "device allocation failed (transposed factor)");
    }
    g->have_lt = false;
    return BOSS_OK;
}
// ... and contents, once per factorisation (the block inverses Dinv2 must be current on stream s)
static void lt_build(boss_gp* g, hipStream_t s) {
    if (g->have_lt) return;
    const int Np = g->Np;
    hipLaunchKernelGGL(transpose_kernel, dim3(Np / 64, Np / 64, 1), dim3(256), 0, s, (const double*)g->A, g->ld, (size_t)0,
                       g->LT, g->ld, (size_t)0, Np);            // same (non power-of-two) leading dimension as the factor
    hipLaunchKernelGGL(transpose_kernel, dim3(PRED_RB / 64, PRED_RB / 64, Np / PRED_RB), dim3(256), 0, s,
                       (const double*)g->Dinv2, PRED_RB, (size_t)PRED_RB * PRED_RB, g->DT2, PRED_RB,
                       (size_t)PRED_RB * PRED_RB, PRED_RB);
    // a = L⁻ᵀ z: 256-row steps from the last to the first (GEMV partials live in the second half of avec's buffer)
    const int nb = Np / PRED_RB;
    double* partial = g->avec + Np;                          // [<= nb-1][256] fits: (nb-1)*256 < Np
    for (int ib = nb - 1; ib >= 0; --ib) {
        const int nch = nb - 1 - ib;
        if (nch > 0)
            hipLaunchKernelGGL(bt_gemv_partial_kernel, dim3(nch), dim3(256), 0, s, (const double*)g->LT, g->ld, ib,
                               (const double*)g->avec, partial);
        hipLaunchKernelGGL(bt_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)g->A, g->ld, Np, g->N, ib, nch,
                           (const double*)partial, (const double*)g->DT2, g->avec);
    }
    g->have_lt = true;
}

struct boss_nlat {
    Ctx* ctx = nullptr;
    int d = 0;
    bool has_noise = false;
    std::vector<unsigned char> discrete;       // d flags (0/1), empty: none
    void* slab = nullptr;                      // descriptors | flags | per GP latent: scaled points, a, 1/λ
    const NlatLatent* desc_dev = nullptr;      // d + 2
    const unsigned char* discrete_dev = nullptr;
};

static bool nlat_same_discrete(const std::vector<unsigned char>& a, const std::vector<unsigned char>& b, int d) {
    for (int k = 0; k < d; ++k)
        if ((!a.empty() && a[k]) != (!b.empty() && b[k])) return false;
    return true;
}

extern "C" int boss_nlat_create(int device, int d, boss_gp_t* const* lam_gps, const double* lam_const, boss_gp_t* amp_gp,
                                double amp_const, boss_gp_t* noise_gp, double noise_const, const int* target,
                                const double* target_par, const int* act, const double* act_par, const unsigned char* discrete,
                                boss_nlat_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || d > NLAT_MAX_D) return fail(BOSS_E_INVALID, "x_dim must be between 1 and 16");
    if (!lam_gps || !lam_const || !target || !target_par || !act || !act_par) return fail(BOSS_E_INVALID, "NULL argument");
    const int nq = d + 2;
    std::vector<boss_gp*> gps(nq);
    std::vector<double> cst(nq);
    for (int q = 0; q < d; ++q) {
        gps[q] = lam_gps[q];
        cst[q] = lam_const[q];
    }
    gps[d] = amp_gp;
    cst[d] = amp_const;
    gps[d + 1] = noise_gp;
    cst[d + 1] = noise_const;
    const bool has_noise = noise_gp || !std::isnan(noise_const);
    for (int q = 0; q < nq; ++q) {
        const boss_gp* g = gps[q];
        if (!g) {
            if (q == d + 1 && !has_noise) continue;
            if (!std::isfinite(cst[q])) return fail(BOSS_E_INVALID, "a constant latent must be finite");
            continue;
        }
        if (g->aug || g->gibbs) return fail(BOSS_E_INVALID, "a latent model must be a plain posterior (boss_gp_create)");
        NOT_FOR_KPROG(g);
        if (g->d != d) return fail(BOSS_E_INVALID, "a latent model's x_dim differs from d");
        if (g->ctx->logical != device) return fail(BOSS_E_INVALID, "a latent model lives on another device");
        if (g->has_mean) return fail(BOSS_E_INVALID, "a latent model with a prior mean cannot be evaluated on the device");
        if (!g->discrete.empty()) return fail(BOSS_E_INVALID, "a latent model must not round dimensions itself");
        if (target[q] < NLAT_T_NONE || target[q] > NLAT_T_UNIFORM) return fail(BOSS_E_INVALID, "unknown target code");
        if (act[q] < NLAT_A_IDENTITY || act[q] > NLAT_A_EXP) return fail(BOSS_E_INVALID, "unknown activation code");
        if (!std::isfinite(target_par[2 * q]) || !std::isfinite(target_par[2 * q + 1]) || !std::isfinite(act_par[q]))
            return fail(BOSS_E_INVALID, "transform parameters must be finite");
    }
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    for (int q = 0; q < nq; ++q)
        if (gps[q] && (rc = gp_settle(gps[q], "a latent model has no valid factorisation")) != BOSS_OK) return rc;
    // descriptors | flags | snapshots (256-byte aligned parts)
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    size_t bytes = al(sizeof(NlatLatent) * nq) + al((size_t)d);
    for (int q = 0; q < nq; ++q)
        if (gps[q]) bytes += al(sizeof(double) * (size_t)d * gps[q]->ldx) + al(sizeof(double) * gps[q]->Np) + al(sizeof(double) * d);
    boss_nlat* L = new boss_nlat();
    L->ctx = c;
    L->d = d;
    L->has_noise = has_noise;
    if (discrete) {
        bool any = false;
        for (int k = 0; k < d; ++k) any |= discrete[k] != 0;
        if (any)
            for (int k = 0; k < d; ++k) L->discrete.push_back(discrete[k] ? 1 : 0);
    }
    if (dev_malloc(&L->slab, bytes) != hipSuccess) {
        delete L;
        return fail(BOSS_E_ALLOC, "device allocation failed");
    }
    char* p = (char*)L->slab;
    L->desc_dev = (const NlatLatent*)p;
    p += al(sizeof(NlatLatent) * nq);
    unsigned char* ddisc = (unsigned char*)p;
    p += al((size_t)d);
    std::vector<NlatLatent> desc(nq);
    hipError_t e = hipSuccess;
    auto keep = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    for (int q = 0; q < nq && rc == BOSS_OK; ++q) {
        NlatLatent& D = desc[q];
        std::memset(&D, 0, sizeof D);
        D.cst = cst[q];
        boss_gp* g = gps[q];
        if (!g) continue;
        // a = (K+σ²I)⁻¹y from the resident factor, as the gradient path forms it
        if ((rc = lt_alloc(g)) != BOSS_OK) break;
        dinv_join(g);
        if (!g->have_dinv) {
            dinv_launch(g, s);
            g->have_dinv = true;
        }
        g->dinv_used = true;
        lt_build(g, s);
        double* xsc = (double*)p;
        p += al(sizeof(double) * (size_t)d * g->ldx);
        double* a = (double*)p;
        p += al(sizeof(double) * g->Np);
        double* il = (double*)p;
        p += al(sizeof(double) * d);
        keep(hipMemcpyAsync(xsc, g->Xsc, sizeof(double) * (size_t)d * g->ldx, hipMemcpyDeviceToDevice, s));
        keep(hipMemcpyAsync(a, g->avec, sizeof(double) * g->Np, hipMemcpyDeviceToDevice, s));
        keep(hipMemcpyAsync(il, g->invlam, sizeof(double) * d, hipMemcpyDeviceToDevice, s));
        D.Xsc = xsc;
        D.a = a;
        D.invlam = il;
        D.N = g->N;
        D.ldx = g->ldx;
        D.kern = g->kernel;
        D.amp2 = g->amp2;
        D.target = target[q];
        D.act = act[q];
        D.tp0 = target_par[2 * q];
        D.tp1 = target_par[2 * q + 1];
        D.ap = act_par[q];
    }
    if (rc == BOSS_OK) {
        keep(hipMemcpyAsync((void*)L->desc_dev, desc.data(), sizeof(NlatLatent) * nq, hipMemcpyHostToDevice, s));
        if (!L->discrete.empty()) {
            keep(hipMemcpyAsync(ddisc, L->discrete.data(), d, hipMemcpyHostToDevice, s));
            L->discrete_dev = ddisc;
        }
    }
    keep(hipStreamSynchronize(s));                           // the snapshot is complete: the handles may change or go
    keep(hipGetLastError());
    if (rc == BOSS_OK && e != hipSuccess) rc = fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    if (rc) {
        (void)hipFree(L->slab);
        delete L;
        return rc;
    }
    *out = L;
    return BOSS_OK;
}

extern "C" void boss_nlat_free(boss_nlat_t* L) {
    if (!L) return;
    if (L->ctx) {
        (void)hipSetDevice(L->ctx->device);
        std::lock_guard<std::mutex> lk(L->ctx->mtx);
        (void)hipStreamSynchronize(L->ctx->stream);
        if (L->slab) (void)hipFree(L->slab);
    }
    delete L;
}

// Enqueue the evaluation of n latent objects at staged candidates Craw [d][Mp] (grid.z = member): member i writes λ to
// clam + i·s_lam, α to camp + i·s_amp, ∂λ/∂x to djl + i·s_jl and ∂α/∂x to dja + i·s_ja (djl, dja null: values only), σ of the
// single object to cnoise (or null).  dbad: the validity flag, set to ~0 here.  Caller holds the context lock.
static int nlat_enqueue(Ctx* c, int n, boss_nlat_t* const* lats, const double* Craw, int Mp, int M, double* clam, size_t s_lam,
                        double* camp, size_t s_amp, double* djl, size_t s_jl, double* dja, size_t s_ja, double* cnoise,
                        unsigned long long* dbad) {
    hipStream_t s = c->stream;
    const boss_nlat* L0 = lats[0];
    const int d = L0->d;
    const bool jac = djl || dja;
    const dim3 block(256);
    (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
    auto job_of = [&](int i) {
        NlatJob j;
        j.lat = lats[i]->desc_dev;
        j.clam = clam + (size_t)i * s_lam;
        j.camp = camp + (size_t)i * s_amp;
        j.cnoise = cnoise;
        j.dlam = djl ? djl + (size_t)i * s_jl : nullptr;
        j.damp = dja ? dja + (size_t)i * s_ja : nullptr;
        return j;
    };
    const int nq = d + 1 + (cnoise ? 1 : 0);
    auto kfn = jac ? nlat_eval_kernel<true> : nlat_eval_kernel<false>;
    if (n == 1) {
        hipLaunchKernelGGL(kfn, dim3(Mp / NLAT_BN, nq, 1), block, 0, s, job_of(0), (const NlatJob*)nullptr, Craw, d, Mp, M,
                           L0->discrete_dev, dbad);
        HIPCHK(hipGetLastError());
        return BOSS_OK;
    }
    int rc = ws_reserve(c->nlatjobs, sizeof(NlatJob) * (size_t)n);
    if (rc) return rc;
    std::vector<NlatJob> jobs(n);
    for (int i = 0; i < n; ++i) jobs[i] = job_of(i);
    const size_t bytes = sizeof(NlatJob) * (size_t)n;
    if (bytes <= PINNED_UP_BYTES) {
        void* stage = (char*)c->pinned + PINNED_UP_OFF;
        HIPCHK(hipEventSynchronize(c->ev_up));
        std::memcpy(stage, jobs.data(), bytes);
        HIPCHK(hipMemcpyAsync(c->nlatjobs.p, stage, bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(c->ev_up, s));
    } else {
        HIPCHK(hipMemcpyAsync(c->nlatjobs.p, jobs.data(), bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    for (int i0 = 0; i0 < n; i0 += 65535) {
        const int cnt = std::min(65535, n - i0);
        hipLaunchKernelGGL(kfn, dim3(Mp / NLAT_BN, nq, cnt), block, 0, s, NlatJob(), (const NlatJob*)c->nlatjobs.p + i0, Craw, d, Mp, M,
                           L0->discrete_dev, dbad);
    }
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

// ... and wait for the flag: an invalid latent value fails the call before anything that reads the buffers is enqueued
static int nlat_check(Ctx* c, const unsigned long long* dbad, long* bad_index) {
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, dbad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    if (bad != ~0ULL) {
        if (bad_index) *bad_index = (long)bad;
        return fail(BOSS_E_INVALID, "latent models: lengthscales must be finite and > 0, amplitudes and noise finite and >= 0");
    }
    return BOSS_OK;
}

constexpr long long NLAT_MAX_JAC = 1LL << 27;               // M·d² doubles of ∂λ/∂x (1 GiB) per object and call

extern "C" int boss_nlat_eval(const boss_nlat_t* L, int M, const double* Xs, double* lam_out, double* amp_out, double* noise_out,
                              double* dlam_out, double* damp_out, long* bad_index) {
    if (!L || !Xs || !lam_out || !amp_out) return fail(BOSS_E_INVALID, "NULL argument");
    if (M < 1) return fail(BOSS_E_INVALID, "M must be >= 1");
    if (bad_index) *bad_index = -1;
    if (noise_out && !L->has_noise) return fail(BOSS_E_INVALID, "the latent object holds no noise model");
    const int d = L->d, Mp = round_up(M, 64);
    if ((long long)M * d * d > NLAT_MAX_JAC) return fail(BOSS_E_INVALID, "M·x_dim² above 2^27 is not supported");
    const bool jac = dlam_out || damp_out;
    Ctx* c = L->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const size_t dMp = (size_t)d * Mp, dm = (size_t)d * M;
    // candidates | λ | α | σ | flag | ∂λ/∂x | ∂α/∂x
    int rc = ws_reserve(c->craw, sizeof(double) * (2 * dMp + 2 * (size_t)Mp + 1 + (jac ? dm * d + dm : 0)));
    if (rc) return rc;
    double* Craw = (double*)c->craw.p;
    double *clam = Craw + dMp, *camp = clam + dMp, *cnoise = camp + Mp;
    unsigned long long* dbad = (unsigned long long*)(cnoise + Mp);
    double *djl = cnoise + Mp + 1, *dja = djl + dm * d;
    std::vector<double> buf;
    pack_points(buf, Xs, d, M, Mp, nullptr);                 // as given: the kernel rounds for λ and α, not for σ
    HIPCHK(hipMemcpyAsync(Craw, buf.data(), sizeof(double) * dMp, hipMemcpyHostToDevice, s));
    boss_nlat_t* one = const_cast<boss_nlat_t*>(L);
    rc = nlat_enqueue(c, 1, &one, Craw, Mp, M, clam, 0, camp, 0, jac ? djl : nullptr, 0, jac ? dja : nullptr, 0,
                      noise_out ? cnoise : nullptr, dbad);
    if (rc == BOSS_OK) rc = nlat_check(c, dbad, bad_index);
    if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    std::vector<double> hl(dMp);
    HIPCHK(hipMemcpyAsync(hl.data(), clam, sizeof(double) * dMp, hipMemcpyDeviceToHost, s));
    std::vector<double> ha(Mp), hn(noise_out ? Mp : 0);
    HIPCHK(hipMemcpyAsync(ha.data(), camp, sizeof(double) * Mp, hipMemcpyDeviceToHost, s));
    if (noise_out) HIPCHK(hipMemcpyAsync(hn.data(), cnoise, sizeof(double) * Mp, hipMemcpyDeviceToHost, s));
    if (dlam_out) HIPCHK(hipMemcpyAsync(dlam_out, djl, sizeof(double) * dm * d, hipMemcpyDeviceToHost, s));
    if (damp_out) HIPCHK(hipMemcpyAsync(damp_out, dja, sizeof(double) * dm, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int j = 0; j < M; ++j) {
        for (int k = 0; k < d; ++k) lam_out[(size_t)j * d + k] = hl[(size_t)k * Mp + j];
        amp_out[j] = ha[j];
        if (noise_out) noise_out[j] = hn[j];
    }
    return BOSS_OK;
}

// What a _lat call checks of its latent objects against its handles (no device work)
static int nlat_match(int n, boss_gp_t* const* gps, boss_nlat_t* const* lats) {
    for (int i = 0; i < n; ++i) {
        const boss_gp* g = gps[i];
        const boss_nlat* L = lats[i];
        if (!L) return fail(BOSS_E_INVALID, "NULL latent object");
        if (L->ctx != g->ctx) return fail(BOSS_E_INVALID, "latent object and posterior live on different devices");
        if (L->d != g->d) return fail(BOSS_E_INVALID, "latent object and posterior differ in x_dim");
        if (!nlat_same_discrete(L->discrete, g->discrete, g->d)) return fail(BOSS_E_INVALID, "latent object and posterior round different dimensions");
    }
    return BOSS_OK;
}
