// host_nfit.inc — the nonstationary likelihood and its gradient in the whitened parameters of the latent ParametrizedGPs
// (boss_nfit_*; nfit_kernels.hpp).  Included by bosship.hip behind host_batch.inc, whose model_loglike_batch_run does the middle:
// this file gives it a parameter block written on the device and a device-side consumer of the cotangents.

struct boss_nfit {
    Ctx* ctx = nullptr;
    int d = 0, N = 0, Nk = 0, nq = 0, T = 0, n_factors = 0;
    std::vector<double> X, y, mean;            // as given (mean empty: none)
    std::vector<unsigned char> discrete;       // d flags or empty
    std::vector<int> factor_of, off;           // per latent: factor index or -1, first row of theta's column
    std::vector<int> nf, slot;                 // per factor: latents sharing it; per latent: its position among them
    NfitDesc desc;                             // transform parameters and mu pointers (col0 / nf are set per chunk)
    void* slab = nullptr;                      // L (Nk×Nk per factor) | Lᵀ (the same) | mu (N per GP latent)
    double *Lf = nullptr, *LTf = nullptr;
    Workspace ws, wpar;                        // chunk buffers of the products; parameter blocks of boss_nfit_values
    std::vector<double> h_up, h_down;          // packed theta of a chunk; its gradients
    // the chunk in flight
    int ctot = 0;
    std::vector<int> fcol0;
    double *TB = nullptr, *YC = nullptr, *GC = nullptr;
};

static void nfit_release(boss_nfit* h) {
    if (h->slab) (void)hipFree(h->slab);
    if (h->ws.p) (void)hipFree(h->ws.p);
    if (h->wpar.p) (void)hipFree(h->wpar.p);
    (void)hipGetLastError();
    delete h;
}

extern "C" int boss_nfit_create(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                                const double* mean_X, int n_factors, const double* factors, const int* factor_of, const double* mu,
                                const int* target, const double* target_par, const int* act, const double* act_par, boss_nfit_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || d > NLAT_MAX_D) return fail(BOSS_E_INVALID, "x_dim must be between 1 and 16");
    if (N < 1 || !X || !y) return fail(BOSS_E_INVALID, "need N >= 1 and non-NULL X, y");
    if (N > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");
    if (n_factors < 0 || (n_factors > 0 && !factors)) return fail(BOSS_E_INVALID, "factors is NULL");
    if (!factor_of || !target || !target_par || !act || !act_par) return fail(BOSS_E_INVALID, "NULL argument");
    const int nq = d + 2;
    for (int q = 0; q < nq; ++q) {
        if (factor_of[q] < -1 || factor_of[q] >= n_factors) return fail(BOSS_E_INVALID, "factor_of: index out of range");
        if (factor_of[q] < 0) continue;
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
    boss_nfit* h = new boss_nfit();
    h->ctx = c;
    h->d = d;
    h->N = N;
    const int Nk = h->Nk = round_up(N, NFIT_BM);
    h->nq = nq;
    h->n_factors = n_factors;
    h->X.assign(X, X + (size_t)d * N);
    h->y.assign(y, y + N);
    if (mean_X) h->mean.assign(mean_X, mean_X + N);
    if (discrete) h->discrete.assign(discrete, discrete + d);
    h->factor_of.assign(factor_of, factor_of + nq);
    h->nf.assign(n_factors, 0);
    h->off.resize(nq);
    h->slot.assign(nq, 0);
    int n_gp = 0;
    for (int q = 0; q < nq; ++q) {
        h->off[q] = h->T;
        const int f = factor_of[q];
        if (f >= 0) {
            h->slot[q] = h->nf[f]++;
            ++n_gp;
        }
        h->T += f >= 0 ? N : 1;
    }
    const size_t fac = (size_t)Nk * Nk, slab_doubles = 2 * fac * n_factors + (size_t)N * n_gp + 8;
    if (dev_malloc(&h->slab, sizeof(double) * slab_doubles) != hipSuccess) {
        h->slab = nullptr;
        nfit_release(h);
        return fail(BOSS_E_ALLOC, "device allocation failed (the latent models' factors do not fit)");
    }
    h->Lf = (double*)h->slab;
    h->LTf = h->Lf + fac * n_factors;
    double* mu_dev = h->LTf + fac * n_factors;
    hipError_t e = hipSuccess;
    auto keep = [&](hipError_t r) {
        if (e == hipSuccess) e = r;
    };
    std::vector<double> hl(fac), ht(fac);
    for (int f = 0; f < n_factors; ++f) {                    // the lower triangle only, zero beyond N, and its transpose
        std::fill(hl.begin(), hl.end(), 0.0);
        std::fill(ht.begin(), ht.end(), 0.0);
        const double* src = factors + (size_t)f * N * N;
        for (int k = 0; k < N; ++k)
            for (int r = k; r < N; ++r) {
                const double v = src[(size_t)k * N + r];
                hl[(size_t)k * Nk + r] = v;
                ht[(size_t)r * Nk + k] = v;
            }
        keep(hipMemcpy(h->Lf + fac * f, hl.data(), sizeof(double) * fac, hipMemcpyHostToDevice));
        keep(hipMemcpy(h->LTf + fac * f, ht.data(), sizeof(double) * fac, hipMemcpyHostToDevice));
    }
    std::memset(&h->desc, 0, sizeof h->desc);
    int g = 0;
    for (int q = 0; q < nq; ++q) {
        NfitLatent& L = h->desc.lat[q];
        if (factor_of[q] < 0) continue;
        L.gp = 1;
        L.target = target[q];
        L.act = act[q];
        L.tp0 = target_par[2 * q];
        L.tp1 = target_par[2 * q + 1];
        L.ap = act_par[q];
        if (mu) {
            L.mu = mu_dev + (size_t)N * g;
            keep(hipMemcpy(mu_dev + (size_t)N * g, mu + (size_t)N * q, sizeof(double) * N, hipMemcpyHostToDevice));
        }
        ++g;
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        nfit_release(h);
        // (BOSS_E_NO_DEVICE is the header's code for every HIP runtime error, as HIPCHK reports them)
        return fail(e == hipErrorOutOfMemory ? BOSS_E_ALLOC : BOSS_E_NO_DEVICE,
                    std::string("HIP runtime error while copying the factors to the device: ") + hipGetErrorString(e));
    }
    *out = h;
    return BOSS_OK;
}

extern "C" void boss_nfit_free(boss_nfit_t* h) {
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    std::lock_guard<std::mutex> lk(h->ctx->mtx);
    (void)hipStreamSynchronize(h->ctx->stream);
    nfit_release(h);
}

extern "C" int boss_nfit_param_count(const boss_nfit_t* h, int* T_out) {
    if (!h || !T_out) return fail(BOSS_E_INVALID, "NULL argument");
    *T_out = h->T;
    return BOSS_OK;
}

// Sets s0 .. s0+nb-1: theta packed and uploaded (once), Y = L Θ per factor, the transform into the parameter blocks par_dev
// (par_doubles apart, rows padded to Np) with the validity flags.  Everything is enqueued on the context's stream; the caller
// synchronises before the next chunk (h_up is reused).  Caller holds the context lock.
static int nfit_stage_enqueue(boss_nfit* h, int s0, int nb, const double* theta, int Np, double* par_dev, size_t par_doubles,
                              int* flags_dev) {
    Ctx* c = h->ctx;
    hipStream_t s = c->stream;
    const int N = h->N, Nk = h->Nk, nq = h->nq, d = h->d;
    h->fcol0.assign(h->n_factors, 0);
    int ctot = 0;
    for (int f = 0; f < h->n_factors; ++f) {
        h->fcol0[f] = ctot;
        ctot += round_up(h->nf[f] * nb, NFIT_BN);
    }
    h->ctot = ctot;
    for (int q = 0; q < nq; ++q) {
        const int f = h->factor_of[q];
        if (f < 0) continue;
        h->desc.lat[q].col0 = h->fcol0[f] + h->slot[q];
        h->desc.lat[q].nf = h->nf[f];
    }
    // theta rows [Nk][ctot] | scalars [nb][nq]   |   Y / V′ [ctot][Nk]   |   G [ctot][Nk] | scalar gradients [nb][nq]
    const size_t nT = (size_t)Nk * ctot, nS = (size_t)nb * nq;
    int rc = ws_reserve(h->ws, sizeof(double) * (3 * nT + 2 * nS + 8));
    if (rc) return rc;
    h->TB = (double*)h->ws.p;
    h->YC = h->TB + nT + nS;
    h->GC = h->YC + nT;
    h->h_up.assign(nT + nS, 0.0);
    for (int b = 0; b < nb; ++b) {
        const double* th = theta + (size_t)(s0 + b) * h->T;
        for (int q = 0; q < nq; ++q) {
            const NfitLatent& L = h->desc.lat[q];
            if (!L.gp) {
                h->h_up[nT + (size_t)b * nq + q] = th[h->off[q]];
                continue;
            }
            double* dst = h->h_up.data() + L.col0 + (size_t)b * L.nf;
            const double* src = th + h->off[q];
            for (int j = 0; j < N; ++j) dst[(size_t)j * ctot] = src[j];
        }
    }
    HIPCHK(hipMemcpyAsync(h->TB, h->h_up.data(), sizeof(double) * (nT + nS), hipMemcpyHostToDevice, s));
    for (int f = 0; f < h->n_factors; ++f) {
        const int cols = round_up(h->nf[f] * nb, NFIT_BN);
        if (cols == 0) continue;
        hipLaunchKernelGGL(nfit_tri_gemm_kernel<false>, dim3(Nk / NFIT_BM, cols / NFIT_BN), dim3(256), 0, s,
                           (const double*)(h->Lf + (size_t)Nk * Nk * f), Nk, (const double*)h->TB, ctot, h->fcol0[f], h->YC);
    }
    for (int b0 = 0; b0 < nb; b0 += 65535)
        hipLaunchKernelGGL(nfit_transform_kernel, dim3(Np / 256 + (Np % 256 != 0), nq, std::min(65535, nb - b0)), dim3(256), 0, s, h->desc, d,
                           N, Np, Nk, h->YC, (const double*)(h->TB + nT), par_dev, par_doubles, flags_dev, b0);
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

extern "C" int boss_nfit_values(boss_nfit_t* h, int S, const double* theta, double* lam_out, double* amp_out, double* noise_out,
                                int* status_out) {
    if (!h || S < 0) return fail(BOSS_E_INVALID, "bad arguments");
    if (S == 0) return BOSS_OK;
    if (!theta || !lam_out || !amp_out || !noise_out) return fail(BOSS_E_INVALID, "NULL argument");
    Ctx* c = h->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const int N = h->N, d = h->d, Np = round_up(N, BLK);
    const size_t par_doubles = ((size_t)d + 2) * Np;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)S, ((size_t)256 << 20) / (par_doubles * sizeof(double))));
    int rc = ws_reserve(h->wpar, sizeof(double) * par_doubles * chunk + sizeof(int) * chunk);
    if (rc) return rc;
    double* par_dev = (double*)h->wpar.p;
    int* flags = (int*)(par_dev + par_doubles * chunk);
    std::vector<double> hp(par_doubles * chunk);
    std::vector<int> hf(chunk);
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int nb = std::min(chunk, S - s0);
        HIPCHK(hipMemsetAsync(flags, 0, sizeof(int) * nb, s));
        if ((rc = nfit_stage_enqueue(h, s0, nb, theta, Np, par_dev, par_doubles, flags)) != BOSS_OK) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        HIPCHK(hipMemcpyAsync(hp.data(), par_dev, sizeof(double) * par_doubles * nb, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hf.data(), flags, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        for (int b = 0; b < nb; ++b) {
            const double* p = hp.data() + (size_t)b * par_doubles;
            const size_t sb = (size_t)(s0 + b);
            for (int j = 0; j < N; ++j) {
                for (int k = 0; k < d; ++k) lam_out[sb * d * N + (size_t)j * d + k] = p[(size_t)k * Np + j];
                amp_out[sb * N + j] = p[(size_t)d * Np + j];
                noise_out[sb * N + j] = p[(size_t)(d + 1) * Np + j];
            }
            if (status_out) status_out[sb] = hf[b] ? BOSS_E_INVALID : BOSS_OK;
        }
    }
    return BOSS_OK;
}

extern "C" int boss_nfit_loglike_grad(boss_nfit_t* h, int S, const double* theta, double* ll_out, double* grad_out, int* status_out) {
    if (!h || S < 0) return fail(BOSS_E_INVALID, "bad arguments");
    if (S == 0) return BOSS_OK;
    if (!theta || !ll_out) return fail(BOSS_E_INVALID, "NULL argument");
    Ctx* c = h->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const int N = h->N, d = h->d, nq = h->nq, Nk = h->Nk, T = h->T;
    const bool grads = grad_out != nullptr;
    const int Np = round_up(N, grads ? PRED_RB : BLK);
    std::vector<double> pts, yb(Np, 0.0);
    pack_points(pts, h->X.data(), d, N, Np, h->discrete.empty() ? nullptr : h->discrete.data());
    std::copy(h->y.begin(), h->y.end(), yb.begin());
    const size_t par_doubles = ((size_t)d + 2) * Np, out_doubles = ((size_t)d + 3) * Np;
    auto gram = [&](const ModelBatchGramArgs& a) { ngp_batch_gram(c, d, N, Np, a); };   // (the array call's launch and view)
    ModelBatchGrad G;
    G.out_doubles = out_doubles;
    G.view = [&](boss_gp* v, const double* pts_dev, double* par) { ngp_batch_view(v, d, Np, pts_dev, par); };
    ModelBatchDevice Dv;
    Dv.fill = [&](int s0, int nb, double* par_dev, int* flags_dev) {
        int rc = nfit_stage_enqueue(h, s0, nb, theta, Np, par_dev, par_doubles, flags_dev);
        if (rc) return rc;
        for (int b0 = 0; b0 < nb; b0 += 65535)
            hipLaunchKernelGGL(nfit_neutralise_kernel, dim3(Np / 256 + (Np % 256 != 0), nq, std::min(65535, nb - b0)), dim3(256), 0, s, N, Np,
                               par_dev, par_doubles, (const int*)flags_dev, b0);
        HIPCHK(hipGetLastError());
        return (int)BOSS_OK;
    };
    if (grads) {
        Dv.consume = [&](int, int nb, const double* sums_dev) {
            const int ctot = h->ctot;
            const size_t nT = (size_t)Nk * ctot, nS = (size_t)nb * nq;
            for (int b0 = 0; b0 < nb; b0 += 65535)
                hipLaunchKernelGGL(nfit_cotangent_kernel, dim3(Nk / 256 + (Nk % 256 != 0), nq, std::min(65535, nb - b0)), dim3(256), 0, s, h->desc,
                                   d, N, Np, Nk, sums_dev, out_doubles, (const double*)h->YC, h->TB, ctot, h->GC + nT, b0);
            for (int f = 0; f < h->n_factors; ++f) {
                const int cols = round_up(h->nf[f] * nb, NFIT_BN);
                if (cols == 0) continue;
                hipLaunchKernelGGL(nfit_tri_gemm_kernel<true>, dim3(Nk / NFIT_BM, cols / NFIT_BN), dim3(256), 0, s,
                                   (const double*)(h->LTf + (size_t)Nk * Nk * f), Nk, (const double*)h->TB, ctot, h->fcol0[f], h->GC);
            }
            HIPCHK(hipGetLastError());
            h->h_down.resize(nT + nS);
            HIPCHK(hipMemcpyAsync(h->h_down.data(), h->GC, sizeof(double) * (nT + nS), hipMemcpyDeviceToHost, s));
            return (int)BOSS_OK;
        };
        Dv.finish = [&](int set, int b, int st) {
            double* gr = grad_out + (size_t)set * T;
            if (st != BOSS_OK) {
                std::fill(gr, gr + T, 0.0);
                return;
            }
            const size_t nT = (size_t)Nk * h->ctot;
            for (int q = 0; q < nq; ++q) {
                const NfitLatent& L = h->desc.lat[q];
                if (!L.gp) gr[h->off[q]] = h->h_down[nT + (size_t)b * nq + q];
                else std::copy_n(h->h_down.data() + (size_t)(L.col0 + b * L.nf) * Nk, N, gr + h->off[q]);
            }
        };
    }
    auto no_fill = [](int, double*) { return false; };
    return model_loglike_batch_run(c, N, Np, S, pts, yb, h->mean.empty() ? nullptr : h->mean.data(), 0, par_doubles, no_fill, gram, ll_out,
                                   status_out, grads ? &G : nullptr, &Dv);
}
