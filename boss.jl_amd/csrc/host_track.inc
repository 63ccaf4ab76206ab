// host_track.inc — tracked candidates (boss_track_*) (included by bosship.hip).

// ------------------------------------------------------------------------------------------
// tracked candidates: resident V slabs, updated in O(N·M) per appended observation
// ------------------------------------------------------------------------------------------
static void track_release(boss_track* t) {
    if (!t) return;
    if (t->ctx) (void)hipSetDevice(t->ctx->device);
    void* ptrs[] = {t->V, t->Csc, t->mu, t->var, t->mean, t->Clam, t->Camp, t->rhs};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete t;
}

// (re)build the whole state with the prediction kernel; caller holds the context lock
static int track_rebuild(boss_track* t, const boss_cand* cd) {
    boss_gp* g = t->gp;
    Ctx* c = t->ctx;
    hipStream_t s = c->stream;
    const int Ncap = g->Np + PRED_RB;
    if (Ncap > t->Ncap) {
        if (t->V) (void)hipFree(t->V);
        t->V = nullptr;
        if (dev_malloc((void**)&t->V, sizeof(double) * (size_t)t->tiles * Ncap * 32) != hipSuccess) {
            (void)hipGetLastError();
            return fail(BOSS_E_ALLOC, "device allocation failed (tracked V slabs)");
        }
        t->Ncap = Ncap;
    }
    int rc;
    if (t->gibbs) {
        // the nonstationary prediction path on the track's own rounded candidates and latent values (cd is not read)
        boss_cand own;
        own.ctx = c;
        own.d = t->d;
        own.M = t->M;
        own.Mp = t->Mp;
        own.Craw = t->Csc;
        rc = predict_enqueue(g, &own, t->has_mean ? t->mean : nullptr, t->mu, t->var, true, t->Clam, t->Camp);
    } else {
        // 32-wide slabs in the scratch; a program kernel's σ² = k(x*, x*) − Σv² + 1e-18 arrives unclipped (kprog_var_launch), its scaled
        // candidates stay in the context's buffer like the built-in kernels'
        rc = predict_enqueue(g, cd, t->has_mean ? t->mean : nullptr, t->mu, t->var, true);
    }
    if (rc) return rc;
    HIPCHK(hipMemcpy2DAsync(t->V, sizeof(double) * (size_t)t->Ncap * 32, c->vscratch.p, sizeof(double) * (size_t)g->Np * 32,
                            sizeof(double) * (size_t)g->Np * 32, t->tiles, hipMemcpyDeviceToDevice, s));
    if (t->aug) {
        HIPCHK(hipMemcpyAsync(t->Csc, cd->Craw, sizeof(double) * (size_t)t->d * t->Mp, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(aug_track_var_kernel, dim3(t->tiles), dim3(256), 0, s, (const double*)t->V, t->Ncap, g->N, t->M, g->amp2, t->var);
        HIPCHK(hipGetLastError());
    } else if (!t->gibbs) {
        HIPCHK(hipMemcpyAsync(t->Csc, c->csc.p, sizeof(double) * (size_t)t->d * t->Mp, hipMemcpyDeviceToDevice, s));
    }
    t->N = g->N;
    t->epoch = g->epoch;
    return BOSS_OK;
}

// A track of any model's posterior at `cand` (the entry points below have checked their arguments).  A pending update is finished
// under the lock; every failure after the track exists goes through one clean-up.  A nonstationary posterior takes λ(x*), α(x*)
// from lam [d][Mp] / amp [Mp], or has its latent models write them into the same buffers (lat): the track keeps them and the
// rounded raw candidates, so gibbs_track_append_kernel can form k_Gibbs(x_r, x*) for every appended row.
static int track_create(boss_gp* g, const boss_cand* cand, const double* lam, const double* amp, const boss_nlat_t* lat,
                        const double* mean_Xs, boss_track_t** out) {
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = gp_settle(g);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const int d = g->d, M = cand->M, Mp = cand->Mp;
    boss_track* t = new boss_track();
    t->ctx = c;
    t->gp = g;
    t->aug = g->aug;
    t->gibbs = g->gibbs;
    t->d = d;
    t->M = M;
    t->Mp = Mp;
    t->tiles = (M + 31) / 32;
    auto bail = [&](int code) {
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        track_release(t);
        return code;
    };
    auto bail_hip = [&](hipError_t e) { return bail(fail(BOSS_E_NO_DEVICE, hipGetErrorString(e))); };
    if (dev_malloc((void**)&t->Csc, sizeof(double) * (size_t)d * Mp) != hipSuccess ||
        (t->gibbs && (dev_malloc((void**)&t->Clam, sizeof(double) * (size_t)d * Mp) != hipSuccess ||
                      dev_malloc((void**)&t->Camp, sizeof(double) * ((size_t)Mp + 1)) != hipSuccess)) ||
        (g->kprog && dev_malloc((void**)&t->rhs, sizeof(double) * (size_t)t->tiles * TRACK_ROWS * 32) != hipSuccess) ||
        dev_malloc((void**)&t->mu, sizeof(double) * M) != hipSuccess ||
        dev_malloc((void**)&t->var, sizeof(double) * M) != hipSuccess ||
        dev_malloc((void**)&t->mean, sizeof(double) * M) != hipSuccess)
        return bail(fail(BOSS_E_ALLOC, "device allocation failed"));
    hipError_t e = hipSuccess;
    if (t->gibbs) {
        hipLaunchKernelGGL(round_cand_kernel, dim3((Mp + 255) / 256), dim3(256), 0, s, (const double*)cand->Craw, t->Csc,
                           (const unsigned char*)g->discrete_dev, d, Mp);
        if (lat) {
            boss_nlat_t* one = const_cast<boss_nlat_t*>(lat);
            unsigned long long* dbad = (unsigned long long*)(t->Camp + Mp);
            rc = nlat_enqueue(c, 1, &one, t->Csc, Mp, M, t->Clam, 0, t->Camp, 0, nullptr, 0, nullptr, 0, nullptr, dbad);
            if (rc == BOSS_OK) rc = nlat_check(c, dbad, nullptr);
            if (rc) return bail(rc);
        } else {
            e = hipMemcpyAsync(t->Clam, lam, sizeof(double) * (size_t)d * Mp, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(t->Camp, amp, sizeof(double) * Mp, hipMemcpyHostToDevice, s);
        }
    }
    if (mean_Xs && e == hipSuccess) {
        e = hipMemcpyAsync(t->mean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s);
        t->has_mean = true;
    }
    if ((t->gibbs || mean_Xs) && e == hipSuccess) e = hipStreamSynchronize(s);   // the caller's arrays may go
    if (e != hipSuccess) return bail_hip(e);
    rc = track_rebuild(t, cand);
    if (rc) return bail(rc);
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return bail_hip(e);
    *out = t;
    return BOSS_OK;
}

extern "C" int boss_track_create(boss_gp_t* g, const boss_cand_t* cand, const double* mean_Xs, boss_track_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!g || !cand) return fail(BOSS_E_INVALID, "NULL argument");
    NOT_FOR_MODELS(g);
    KPROG_NEEDS_SEQ(g);
    if (cand->ctx != g->ctx || cand->d != g->d) return fail(BOSS_E_INVALID, "candidates and posterior must share device and x_dim");
    return track_create(g, cand, nullptr, nullptr, nullptr, mean_Xs, out);
}

// Tracked candidates of a nonstationary posterior: the prediction runs once through the nonstationary path (unclipped moments);
// λ(x*), α(x*) come from the caller's arrays, checked and padded here, or from the latent models on the device (lat).
constexpr int NGP_TRACK_MAX_D = 16;
static int ngp_track_create(boss_gp_t* g, const boss_cand_t* cand, const double* lam_Xs, const double* amp_Xs, const boss_nlat_t* lat,
                            const double* mean_Xs, boss_track_t** out) {
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    if (g->d > NGP_TRACK_MAX_D) return fail(BOSS_E_INVALID, "tracked candidates of nonstationary posteriors support x_dim <= 16");
    if (cand->ctx != g->ctx || cand->d != g->d) return fail(BOSS_E_INVALID, "candidates and posterior must share device and x_dim");
    const int d = g->d, M = cand->M, Mp = cand->Mp;
    std::vector<double> lam, amp;
    if (lat) {
        boss_nlat_t* one = const_cast<boss_nlat_t*>(lat);
        int rc = nlat_match(1, &g, &one);
        if (rc) return rc;
    } else {
        lam.assign((size_t)d * Mp, 1.0);                     // (checked and padded as ngp_pack does)
        amp.assign(Mp, 0.0);
        for (int j = 0; j < M; ++j) {
            for (int k = 0; k < d; ++k) {
                const double v = lam_Xs[(size_t)j * d + k];
                if (!(v > 0.0) || !std::isfinite(v)) return fail(BOSS_E_INVALID, "lengthscales must be finite and > 0");
                lam[(size_t)k * Mp + j] = v;
            }
            if (!(amp_Xs[j] >= 0.0) || !std::isfinite(amp_Xs[j])) return fail(BOSS_E_INVALID, "amplitudes must be finite and >= 0");
            amp[j] = amp_Xs[j];
        }
    }
    return track_create(g, cand, lam.data(), amp.data(), lat, mean_Xs, out);
}
extern "C" int boss_ngp_track_create(boss_gp_t* g, const boss_cand_t* cand, const double* lam_Xs, const double* amp_Xs,
                                     const double* mean_Xs, boss_track_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!g || !cand || !lam_Xs || !amp_Xs) return fail(BOSS_E_INVALID, "NULL argument");
    return ngp_track_create(g, cand, lam_Xs, amp_Xs, nullptr, mean_Xs, out);
}
extern "C" int boss_ngp_track_create_lat(boss_gp_t* g, const boss_cand_t* cand, const boss_nlat_t* lat, const double* mean_Xs,
                                         boss_track_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!g || !cand || !lat) return fail(BOSS_E_INVALID, "NULL argument");
    return ngp_track_create(g, cand, nullptr, nullptr, lat, mean_Xs, out);
}

// Tracked candidates of a gradient-observation posterior: the V slabs come from the model's own prediction path, the raw
// candidates stay resident so aug_track_append_kernel can form the cross-covariance of every appended row.
extern "C" int boss_ggp_track_create(boss_gp_t* g, const boss_cand_t* cand, boss_track_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!g || !cand) return fail(BOSS_E_INVALID, "NULL argument");
    if (!g->aug) return fail(BOSS_E_INVALID, "handle was not created by boss_ggp_create");
    if (cand->ctx != g->ctx || cand->d != g->d) return fail(BOSS_E_INVALID, "candidates and posterior must share device and x_dim");
    return track_create(g, cand, nullptr, nullptr, nullptr, nullptr, out);
}

extern "C" void boss_track_free(boss_track_t* t) {
    if (!t) return;
    if (t->ctx) {
        (void)hipSetDevice(t->ctx->device);
        (void)hipStreamSynchronize(t->ctx->stream);
    }
    track_release(t);
}

// bring the state up to the posterior's current N (enqueue only); caller holds the context lock
static int track_sync_locked(boss_track* t) {
    boss_gp* g = t->gp;
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "the tracked posterior has no valid factorisation");
    if (t->epoch != g->epoch)
        return fail(BOSS_E_INVALID, "the tracked posterior was re-fitted with new hyper-parameters: create a new track");
    if (g->N < t->N) return fail(BOSS_E_INVALID, "the tracked posterior shrank");
    if (g->N > t->Ncap) return fail(BOSS_E_INVALID, "tracked state out of capacity: create a new track");
    hipStream_t s = t->ctx->stream;
    for (int N0 = t->N; N0 < g->N; N0 += TRACK_ROWS) {
        const int n = std::min(TRACK_ROWS, g->N - N0);
        if (t->aug)
            hipLaunchKernelGGL(aug_track_append_kernel, dim3(t->tiles), dim3(256), sizeof(double) * (t->d * 32 + t->d), s, (const double*)g->A,
                               g->ld, g->Np, N0, n, t->V, t->Ncap, (const double*)g->Xraw, g->ldx, g->nhead, (const double*)t->Csc, t->d,
                               t->Mp, t->M, g->kernel, g->amp2, (const double*)g->invlam, t->mu, t->var);
        else if (t->gibbs)
            hipLaunchKernelGGL(gibbs_track_append_kernel, dim3(t->tiles), dim3(256), sizeof(double) * (2 * t->d + 1) * 32, s,
                               (const double*)g->A, g->ld, g->Np, N0, n, t->V, t->Ncap, (const double*)g->Xraw, (const double*)g->lamX,
                               (const double*)g->ampX, g->Np, (const double*)t->Csc, (const double*)t->Clam, (const double*)t->Camp,
                               t->d, t->Mp, t->M, t->mu, t->var);
        else if (g->kprog) {
            // the program's right-hand sides first (its interpreter needs a workgroup shape of its own), then the shared pass over V
            kprog_track_rhs_launch(g, N0, n, t->Csc, t->Mp, t->M, t->tiles, t->rhs, s);
            hipLaunchKernelGGL(track_append_kernel<true>, dim3(t->tiles), dim3(256), 0, s, (const double*)g->A, g->ld, g->Np, N0, n, t->V,
                               t->Ncap, (const double*)g->Xsc, g->Np, (const double*)t->Csc, t->d, t->Mp, t->M, g->kernel, g->amp2,
                               t->mu, t->var, (const double*)t->rhs);
        } else
            hipLaunchKernelGGL(track_append_kernel<false>, dim3(t->tiles), dim3(256), 0, s, (const double*)g->A, g->ld, g->Np, N0, n, t->V,
                               t->Ncap, (const double*)g->Xsc, g->Np, (const double*)t->Csc, t->d, t->Mp, t->M, g->kernel, g->amp2,
                               t->mu, t->var, (const double*)nullptr);
    }
    t->N = g->N;
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

extern "C" int boss_track_sync(boss_track_t* t) {
    if (!t) return fail(BOSS_E_INVALID, "track is NULL");
    Ctx* c = t->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = track_sync_locked(t);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return BOSS_OK;
}

extern "C" int boss_track_moments(boss_track_t* t, int first, int count, double* mu, double* var) {
    if (!t || !mu || !var || first < 0 || count < 1 || first + count > t->M) return fail(BOSS_E_INVALID, "bad arguments");
    Ctx* c = t->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = track_sync_locked(t);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(mu, t->mu + first, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(var, t->var + first, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (t->aug)                                              // the reference's max(0, ·); the resident value stays unclipped
        for (int i = 0; i < count; ++i) var[i] = std::max(0.0, var[i]);
    return BOSS_OK;
}

extern "C" int boss_acq_ei_tracks(int P, int S, boss_track_t* const* tracks, const double* fit_coefs, const double* y_max,
                                  int has_best, double best, const unsigned char* valid_mask, double* acq_out,
                                  long* argmax_out, double* max_out) {
    if (P < 1 || S < 1 || !tracks || !fit_coefs) return fail(BOSS_E_INVALID, "bad arguments");
    for (int i = 0; i < P * S; ++i) {
        if (!tracks[i]) return fail(BOSS_E_INVALID, "NULL track");
        if (tracks[i]->ctx != tracks[0]->ctx || tracks[i]->M != tracks[0]->M)
            return fail(BOSS_E_INVALID, "all tracks must share the device and the candidate set");
    }
    Ctx* c = tracks[0]->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const int M = tracks[0]->M;
    const size_t nd = (size_t)2 * P * M + M + 2 * P;
    int rc = ws_reserve(c->acq, sizeof(double) * nd + M);
    if (rc) return rc;
    double* dev = (double*)c->acq.p;
    double* dmu = dev;
    double* dvar = dmu + (size_t)P * M;
    double* dacq = dvar + (size_t)P * M;
    double* dcoef = dacq + M;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(dev + nd);
    double* hres = (double*)c->pinned;
    EiPar par;
    rc = ei_params(c, s, P, fit_coefs, y_max, has_best, best, &par, dcoef, dymax);
    if (rc) return rc;
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    if (S > 1) (void)hipMemsetAsync(dacq, 0, sizeof(double) * M, s);
    for (int sm = 0; sm < S; ++sm) {
        for (int p = 0; p < P; ++p) {
            boss_track* t = tracks[p + (size_t)P * sm];
            rc = track_sync_locked(t);
            if (rc) {
                (void)hipStreamSynchronize(s);
                return rc;
            }
            (void)hipMemcpyAsync(dmu + (size_t)p * M, t->mu, sizeof(double) * M, hipMemcpyDeviceToDevice, s);
            (void)hipMemcpyAsync(dvar + (size_t)p * M, t->var, sizeof(double) * M, hipMemcpyDeviceToDevice, s);
            if (t->aug) hipLaunchKernelGGL(clip_nonneg_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dvar + (size_t)p * M, M);
        }
        if (sm + 1 < S)
            hipLaunchKernelGGL(ei_accumulate_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dmu, dvar, M, M, par, dcoef, dymax,
                               dacq);
        else
            hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, dmu, dvar, M, M, par, dcoef, dymax,
                               dacq, S > 1 ? 1 : 0, 1.0 / S, valid_mask ? dmask : nullptr, hres, 0ull);
    }
    if (acq_out) (void)hipMemcpyAsync(acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
    if (max_out) *max_out = hres[0];
    return BOSS_OK;
}
