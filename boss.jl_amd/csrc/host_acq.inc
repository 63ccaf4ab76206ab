// host_acq.inc — EI × feasibility entry points and the likelihood gradient (included by bosship.hip).

// ------------------------------------------------------------------------------------------
// acquisition
// ------------------------------------------------------------------------------------------
// dpair / idx_off / defer: one shard of a multi-device call (host_multi.inc) — the epilogue also leaves (max, global index) in the
// device buffer dpair, and with defer the call returns right behind the enqueue (the caller runs the exchange on the same stream and
// waits once); the shard's own (max, index) are then read from the context's pinned block by acq_shard_result.
// The prediction stays this function's own (the arg-max-only attempt, the deferred shard, the caller's mean layout and the per-sample
// loop on P×M scratch); whether the set launches are taken is members_set_path's answer, the set branch ends in the shared epilogue.
static int acq_ei_impl(int P, int S, boss_gp_t* const* gps, const boss_cand_t* cand, const double* mean_Xs,
                       const double* fit_coefs, const double* y_max, int has_best, double best,
                       const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out,
                       double* dpair, long idx_off, bool defer, const McEpi* mc = nullptr, const AcqpEpi* pg = nullptr) {
    // mc: the EI term is the Monte-Carlo mean of a fitness program (boss_acq_ei_mc, host_fitness.inc) — fit_coefs is not read, P <= EI_MAXP
    // pg: an acquisition program over the moments in the place of EI (boss_acq_prog, host_acqprog.inc) — the caller passes has_best = 1
    //     (mode != 0: the predictions run), fit_coefs / y_max / best are not read, P <= ACQP_MAXP, every handle kind of the EI call
    if (P < 1 || S < 1 || !gps || !cand || (!fit_coefs && !mc && !pg)) return fail(BOSS_E_INVALID, "bad arguments");
    Ctx* c = cand->ctx;
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < P * S; ++i) {
        if (!gps[i]) return fail(BOSS_E_INVALID, "NULL posterior handle");
        if (gps[i]->ctx != c) return fail(BOSS_E_INVALID, "all handles and candidates must live on one device");
        if (mc) NOT_FOR_KPROG(gps[i]);                       // (Monte-Carlo EI: built-in kernels only; the multi-device callers refuse such handles themselves)
        if (!gps[i]->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    }
    std::lock_guard<std::mutex> lk(c->mtx);                 // the per-device scratch areas are shared
    hipStream_t s = c->stream;
    const int M = cand->M;
    // device scratch: mu[P][M] | var[P][M] | acq[M] | mean[P][M] | coefs[P] | ymax[P] | mask
    const size_t nd = (size_t)3 * P * M + M + 2 * P;
    {
        int rc = ws_reserve(c->acq, sizeof(double) * nd + M);      // grow-only: no hipMalloc/hipFree (= device sync) per call
        if (rc) return rc;
    }
    double* dev = (double*)c->acq.p;
    double* dmu = dev;
    double* dvar = dmu + (size_t)P * M;
    double* dacq = dvar + (size_t)P * M;
    double* dmean = dacq + M;
    double* dcoef = dmean + (size_t)P * M;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(dev + nd);
    // written by the epilogue kernel (mapped host memory).  A deferred shard of a multi-device call is read by its caller AFTER this
    // function has released the context's lock: it gets an area of its own, which only multi-device calls (serialised by their own
    // lock) write — a boss_acq_ei on the same context from another thread in that window cannot overwrite it
    double* hres = (double*)c->pinned + (defer ? MULTI_RES_OFF : 0);
    EiPar par;
    const double no_coefs[EI_MAXP] = {};
    int rc = ei_params(c, s, P, (mc || pg) ? no_coefs : fit_coefs, y_max, has_best, best, &par, dcoef, dymax);
    if (rc) return rc;
    const double* deps = nullptr;
    if (mc) {
        rc = mc_stage(c, s, P, *mc, &deps);
        if (rc) return rc;
    }
    EiPar par0 = par;                                        // (mode 0: acq_epilogue_kernel adds 0.0 to the sums the Monte-Carlo kernel left)
    par0.mode = 0;
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    if (!acq_out && !defer) {
        // arg-max only: bound every candidate, finish the contenders (host_prune.inc); anything it declines runs the full kernel below
        for (int i = 0; i < 5; ++i) c->prune_last[i] = 0;
        if (prune_eligible(gps[0], cand, P, S, par, acq_out != nullptr, defer, mc != nullptr || pg != nullptr, dpair)) {
            if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s);   // (P = S = 1: the caller's layout is [j])
            bool done = false;
            double pmax = 0.0;
            long pidx = 0;
            rc = acq_prune_try(gps[0], cand, mean_Xs ? dmean : nullptr, valid_mask ? dmask : nullptr, par, &done, &pmax, &pidx);
            if (rc) return rc;
            if (done) {
                if (argmax_out) *argmax_out = pidx;
                if (max_out) *max_out = pmax;
                return BOSS_OK;
            }
        }
    }
    std::vector<double> hmean;
    const bool set_path = members_set_path(P * S, gps, cand, S > 1 && par.mode != 0, false, false);
    if (S > 1 && !set_path) (void)hipMemsetAsync(dacq, 0, sizeof(double) * M, s);
    if (set_path) {
        // Bayesian-inference average over S posteriors of one shape: ALL P·S predictions in one launch (grid = candidate tiles ×
        // posteriors), moments [s][p][j] resident, then the EI sum over the samples in sample order and the usual epilogue
        const size_t pm = (size_t)P * M;
        rc = ws_reserve(c->setmom, sizeof(double) * pm * S * (mean_Xs ? 3 : 2));
        if (rc) return rc;
        double* mu_all = (double*)c->setmom.p;
        double* var_all = mu_all + pm * S;
        double* mean_all = mean_Xs ? var_all + pm * S : nullptr;
        if (mean_Xs) {
            // caller layout p + P*(j + M*s)  ->  device [s][p][j]
            hmean.resize(pm * S);
            for (int sm = 0; sm < S; ++sm)
                for (int j = 0; j < M; ++j)
                    for (int p = 0; p < P; ++p) hmean[pm * sm + (size_t)p * M + j] = mean_Xs[p + (size_t)P * (j + (size_t)M * sm)];
            (void)hipMemcpyAsync(mean_all, hmean.data(), sizeof(double) * pm * S, hipMemcpyHostToDevice, s);
            (void)hipStreamSynchronize(s);
        }
        rc = predict_set_enqueue(P * S, gps, cand, mean_all, mu_all, var_all, (size_t)M);   // posterior p + P·s -> offset (p + P·s)·M = [s][p][·]
        if (rc) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        ei_value_epilogue_launch(s, mu_all, var_all, M, S, par, dcoef, dymax, valid_mask ? dmask : nullptr, mc, deps, dacq, hres,
                                 (acq_out || defer) ? 0ull : ++c->acq_seq, dpair, idx_off, pg);
    } else
    for (int sm = 0; sm < S; ++sm) {
        if (par.mode != 0) {
            if (mean_Xs) {
                // caller layout p + P*(j + M*s)  →  device [p][j]
                hmean.resize((size_t)P * M);
                for (int j = 0; j < M; ++j)
                    for (int p = 0; p < P; ++p) hmean[(size_t)p * M + j] = mean_Xs[p + (size_t)P * (j + (size_t)M * sm)];
                (void)hipMemcpyAsync(dmean, hmean.data(), sizeof(double) * P * M, hipMemcpyHostToDevice, s);
                (void)hipStreamSynchronize(s);
            }
            for (int p = 0; p < P; ++p) {
                rc = predict_enqueue(gps[p + (size_t)P * sm], cand, mean_Xs ? dmean + (size_t)p * M : nullptr,
                                     dmu + (size_t)p * M, dvar + (size_t)p * M);
                if (rc) {
                    (void)hipStreamSynchronize(s);
                    return rc;
                }
            }
        }
        ProfScope ps(c, sm + 1 < S ? "ei" : "argmax");
        if (pg) {
            // this sample's program value into the sums; behind the last one the mean, the mask (to pg->outside) and the arg-max
            acqp_accumulate_launch(s, dmu, dvar, 0, M, M, 0, 1, *pg, dacq, sm > 0 ? 1 : 0);
            if (sm + 1 == S)
                hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, dmu, dvar, M, M, par0, dcoef, dymax, dacq, 2, 1.0 / S,
                                   valid_mask ? dmask : nullptr, hres, (acq_out || defer) ? 0ull : ++c->acq_seq, dpair, idx_off, pg->outside);
        } else if (mc) {
            // this sample's Monte-Carlo term (BI: its own ε column) into the sums; behind the last one the mean, the mask and the arg-max
            mc_accumulate_launch(s, dmu, dvar, 0, M, M, 0, 1, S, par, *mc, S > 1 ? deps + (size_t)sm * P : deps, dacq, sm > 0 ? 1 : 0);
            if (sm + 1 == S)
                hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, dmu, dvar, M, M, par0, dcoef, dymax, dacq, 1, 1.0 / S,
                                   valid_mask ? dmask : nullptr, hres, (acq_out || defer) ? 0ull : ++c->acq_seq, dpair, idx_off);
        } else if (sm + 1 < S)
            hipLaunchKernelGGL(ei_accumulate_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dmu, dvar, M, M, par, dcoef, dymax,
                               dacq);
        else                                                 // last sample: EI + BI average + mask + arg-max in one launch
            hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, dmu, dvar, M, M, par, dcoef, dymax,
                               dacq, S > 1 ? 1 : 0, 1.0 / S, valid_mask ? dmask : nullptr, hres, (acq_out || defer) ? 0ull : ++c->acq_seq,
                               dpair, idx_off);
    }
    if (acq_out) (void)hipMemcpyAsync(acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, s);
    if (defer) {
        hipError_t e0 = hipGetLastError();
        return e0 == hipSuccess ? BOSS_OK : fail(BOSS_E_NO_DEVICE, hipGetErrorString(e0));
    }
    bool got = false;
    if (!acq_out) {
        // arg-max only: the epilogue kernel writes {max, arg-max, this call's sequence number} into the pinned result block; polling
        // that word returns 10-20 µs before the stream's completion signal would
        volatile unsigned long long* seq = reinterpret_cast<volatile unsigned long long*>(hres) + 2;
        for (unsigned long i = 1;; ++i) {
            if (*seq == c->acq_seq) {
                got = true;
                break;
            }
            if ((i & 0x3fff) == 0 && hipStreamQuery(s) != hipErrorNotReady) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    hipError_t e = got ? hipSuccess : hipStreamSynchronize(s);
    hipError_t e2 = hipGetLastError();
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e2));
    if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
    if (max_out) *max_out = hres[0];
    return BOSS_OK;
}

extern "C" int boss_acq_ei(int P, int S, boss_gp_t* const* gps, const boss_cand_t* cand, const double* mean_Xs,
                           const double* fit_coefs, const double* y_max, int has_best, double best,
                           const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    return acq_ei_impl(P, S, gps, cand, mean_Xs, fit_coefs, y_max, has_best, best, valid_mask, acq_out, argmax_out, max_out, nullptr, 0, false);
}

// EI x feasibility from posterior moments that are already on the host (outputs fitted on other
// ranks and all-gathered, SURVEY 8e "outputs"): the same K8/K9 epilogue kernels as boss_acq_ei.
extern "C" int boss_acq_ei_moments(int device, int P, int S, int M, const double* mu, const double* var,
                                   const double* fit_coefs, const double* y_max, int has_best, double best,
                                   const unsigned char* valid_mask, double* acq_out, long* argmax_out,
                                   double* max_out) {
    if (P < 1 || S < 1 || M < 1 || !mu || !var || !fit_coefs) return fail(BOSS_E_INVALID, "bad arguments");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const size_t pm = (size_t)P * M;
    const size_t nd = 2 * pm * S + M + 2 * P;
    rc = ws_reserve(c->acq, sizeof(double) * nd + M);
    if (rc) return rc;
    double* dev = (double*)c->acq.p;
    double* dmu = dev;
    double* dvar = dmu + pm * S;
    double* dacq = dvar + pm * S;
    double* dcoef = dacq + M;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(dev + nd);
    double* hres = (double*)c->pinned;
    EiPar par;
    rc = ei_params(c, s, P, fit_coefs, y_max, has_best, best, &par, dcoef, dymax);
    if (rc) return rc;
    (void)hipMemcpyAsync(dmu, mu, sizeof(double) * pm * S, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(dvar, var, sizeof(double) * pm * S, hipMemcpyHostToDevice, s);
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    ei_value_epilogue_launch(s, dmu, dvar, M, S, par, dcoef, dymax, valid_mask ? dmask : nullptr, nullptr, nullptr, dacq, hres, 0ull);
    if (acq_out) (void)hipMemcpyAsync(acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
    if (max_out) *max_out = hres[0];
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// gradient of the log marginal likelihood w.r.t. (lengthscale[d], amplitude, noise_std) at the
// hyper-parameters of the last boss_gp_update (SURVEY §8f3)
// ------------------------------------------------------------------------------------------
// Device part for one factorised posterior (a handle, or a view into a batch): Σ-vector {S_1..S_d, tr K⁻¹, ‖a‖²} into
// sums_out (device, d+2 doubles).  The per-device workspaces are reused call after call: everything runs in order on s.
static int llgrad_enqueue(boss_gp* g, hipStream_t s, double* sums_out, int bank, const SetBatch& B, const double* amp2_dev,
                          int amp2_stride, const MeanFold* mf) {
    // mf: null, or where a = K⁻¹(y − m) and its fold with the mean's Jacobian go (mean_fold_kernel, right behind the partials of a on
    //    the same stream: the bank's workspace is not reused before it has run);
    // bank: which set of workspaces (the batched entry point rotates large sets over several streams);
    // B: nb equally shaped posteriors behind g's pointers (small sets: every launch covers the whole group in grid.z),
    //    α² of set b at amp2_dev[b · amp2_stride], its Σ-vector at sums_out + b (d+2); the gradient-observation model's sets have
    //    their parameter blocks B.sPar apart behind g->invlam / g->hyp and d+3 sums each, the nonstationary model's their latent
    //    values B.sPar apart behind g->lamX / g->ampX / g->noiseX and (d+3)·Np results each
    Ctx* c = g->ctx;
    const int d = g->d, N = g->N, Np = g->Np, ld = g->ld, nb = B.nb;
    const int nt = Np / 64, ntiles = nt * (nt + 1) / 2, nv = g->aug ? d + 3 : d + 2, nch = 8;   // (gradient-observation model: λ[d], α-sum, two traces)
    const int gibbs_js = std::max(1, std::min(16, Np / 64));      // column splits of the nonstationary model's row sums (4 partial slots each)
    const size_t sW = (size_t)ld * Np,
                 sC = (size_t)nch * Np + (g->gibbs ? (size_t)gibbs_js * 4 * (d + 1) * Np : (size_t)ntiles * nv);
    Workspace &wA = bank ? c->lgbank[bank - 1][0] : c->lgA, &wB = bank ? c->lgbank[bank - 1][1] : c->lgB,
              &wC = bank ? c->lgbank[bank - 1][2] : c->lgC;
    int rc = ws_reserve(wA, sizeof(double) * sW * nb);
    if (rc) return rc;
    rc = ws_reserve(wB, sizeof(double) * sW * nb);
    if (rc) return rc;
    rc = ws_reserve(wC, sizeof(double) * sC * nb);
    if (rc) return rc;
    double* LinvT = (double*)wA.p;
    double* Kinv = (double*)wB.p;
    double* apart = (double*)wC.p;
    double* parts = apart + (size_t)nch * Np;
    SetBatch Bw = B;
    Bw.sW = nb > 1 ? sW : 0;
    dinv_join(g);
    if (!g->have_dinv) {
        dinv_launch(g, s, B);
        g->have_dinv = true;
    }
    g->dinv_used = true;
    typedef PredG32 G;
    static const bool linvt_solve = getenv("BOSS_LINVT_SOLVE") && atoi(getenv("BOSS_LINVT_SOLVE"));   // A/B: the substitution
    if (linvt_solve && nb == 1) {
        hipLaunchKernelGGL(linvt_kernel<G>, dim3(Np / 32), dim3(G::NTHREADS), PredictLds<G>::BYTES, s, (const double*)g->A, ld, Np,
                           (const double*)g->Dinv2, LinvT, ld);
    } else {
        // L⁻ᵀ by recursive doubling (see linv_level_kernel); the lower work matrix lives in the buffer K⁻¹ overwrites afterwards
        linv_enqueue(g, s, LinvT, Kinv, Bw);
    }
    hipLaunchKernelGGL(kinv_syrk_kernel<SyrkG>, dim3(g->nblk * (g->nblk + 1) / 2, 1, nb), dim3(256), 0, s, (const double*)LinvT, ld, Np,
                       Kinv, ld, Bw.sW);
    hipLaunchKernelGGL(avec_partial_kernel, dim3(Np / 256, nch, nb), dim3(256), 0, s, (const double*)LinvT, ld, Np, N,
                       (const double*)g->A, ld, apart, Bw.sW, B.sA, nb > 1 ? sC : (size_t)0);
    if (mf && (mf->dmean || (mf->dtheta && mf->T > 0))) {
        const int T = mf->dtheta ? mf->T : 0;
        hipLaunchKernelGGL(mean_fold_kernel, dim3(std::max(1, (T + MFOLD_COLS - 1) / MFOLD_COLS), 1, nb), dim3(MFOLD_THREADS), 0, s,
                           (const double*)apart, nch, Np, N, T ? mf->J : (const double*)nullptr, T, mf->dmean, T ? mf->dtheta : (double*)nullptr,
                           nb > 1 ? sC : (size_t)0, mf->sJ);
    }
    const size_t zC = nb > 1 ? sC : (size_t)0, zPar = nb > 1 ? B.sPar : (size_t)0;
    if (g->gibbs) {
        // per-point partial derivatives (boss_ngp_loglike_grad): sums_out holds (d + 3) rows of Np per set
        hipLaunchKernelGGL(mirror_lower_kernel, dim3(Np / 64, Np / 64, nb), dim3(256), 0, s, Kinv, ld, Np, Bw.sW);
        hipLaunchKernelGGL(mirror_diag_kernel, dim3(Np / 64, 1, nb), dim3(256), 0, s, Kinv, ld, Bw.sW);
        hipLaunchKernelGGL(gibbs_llgrad_kernel, dim3(Np / 64, gibbs_js, nb), dim3(256), 0, s, (const double*)g->Xraw, (const double*)g->lamX,
                           (const double*)g->ampX, d, N, Np, (const double*)Kinv, ld, (const double*)apart, nch, parts, zPar, Bw.sW, zC);
        hipLaunchKernelGGL(gibbs_llgrad_reduce_kernel, dim3((Np + 255) / 256, 1, nb), dim3(256), 0, s, (const double*)parts, gibbs_js * 4, d, N,
                           Np, (const double*)g->noiseX, (const double*)Kinv, ld, (const double*)apart, nch, sums_out, zPar, Bw.sW, zC,
                           nb > 1 ? (size_t)(d + 3) * Np : (size_t)0);
        return BOSS_OK;
    }
    if (g->aug)
        hipLaunchKernelGGL(aug_llgrad_tile_kernel, dim3(ntiles, 1, nb), dim3(256), 0, s, (const double*)g->Xraw, g->ldx, d, g->nhead, N, Np,
                           g->kernel, (const double*)g->hyp, (const double*)g->invlam, zPar, (const double*)Kinv, ld, (const double*)apart, nch,
                           parts, Bw.sW, zC);
    else if (g->kprog)
        kprog_llgrad_launch(g, s, ntiles, Kinv, apart, nch, parts);   // (one posterior: the batched calls are built-in only)
    else
    hipLaunchKernelGGL(llgrad_tile_kernel, dim3(ntiles, 1, nb), dim3(256), 0, s, (const double*)g->Xsc, d, N, Np, g->kernel, amp2_dev,
                       amp2_stride, (const double*)Kinv, ld, (const double*)apart, nch, parts, B.sX, Bw.sW, nb > 1 ? sC : (size_t)0,
                       nb > 1 ? sC : (size_t)0);
    hipLaunchKernelGGL(llgrad_reduce_kernel, dim3(nv, 1, nb), dim3(256), 0, s, (const double*)parts, ntiles, nv, sums_out,
                       nb > 1 ? sC : (size_t)0, (size_t)nv);
    return BOSS_OK;
}

// ∂ℓ/∂(λ_1..λ_d, α, σ) from the Σ-vector h; invlam = 1/(λ+1e-8), amp2 = (α+1e-8)², sig2 = (σ+1e-8)²
static void llgrad_finalize(int d, int N, const double* invlam, double amp2, double sig2, double zz, const double* h, double* grad_out) {
    const double amp = std::sqrt(amp2), sig = std::sqrt(sig2), trK = h[d], aa = h[d + 1];
    for (int m = 0; m < d; ++m) grad_out[m] = -h[m] * invlam[m];                       // −S_m / λ_m
    grad_out[d] = (zz - N - sig2 * (aa - trK)) / amp;
    grad_out[d + 1] = sig * (aa - trK);
}

// The sums of one fitted handle on the host (h.size() doubles, see llgrad_enqueue): through the context's prediction workspace, one
// copy back, one synchronisation.  n_mean > 0: the last n_mean doubles of h receive a = K⁻¹(y − m).  Caller holds the context's lock.
static int llgrad_download(boss_gp* g, std::vector<double>& h, size_t n_mean = 0) {
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    int rc = ws_reserve(c->pred, sizeof(double) * h.size());
    if (rc) return rc;
    double* sums = (double*)c->pred.p;
    MeanFold mf;
    if (n_mean) mf.dmean = sums + (h.size() - n_mean);
    rc = llgrad_enqueue(g, s, sums, 0, SetBatch(), g->gibbs ? (const double*)nullptr : (const double*)g->hyp, 0, n_mean ? &mf : nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(h.data(), sums, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

extern "C" int boss_gp_loglike_grad(boss_gp_t* g, double* logpdf_out, double* grad_out) {
    if (!g || !grad_out) return fail(BOSS_E_INVALID, "NULL argument");
    NOT_FOR_MODELS(g);
    KPROG_NEEDS_GRAD(g);
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = gp_settle(g);
    if (rc) return rc;
    const int d = g->d, nv = d + 2;
    if (d > LLG_MAX_D) return fail(BOSS_E_INVALID, "x_dim too large for the likelihood-gradient kernel");
    hipStream_t s = c->stream;
    if (small_fit_ok(c, g->N, d) && !g->gibbs && !g->kprog) {
        // N <= 128: one workgroup, one launch, the Σ-vector lands in mapped host memory (small_llgrad_kernel)
        dinv_join(g);
        hipLaunchKernelGGL(small_llgrad_kernel, dim3(1), dim3(DIAG_THREADS), SMALL_LLG_LDS_BYTES, s, (const double*)g->A, g->ld, g->Np,
                           g->N, d, g->kernel, g->amp2, (const double*)g->inv16, (const double*)g->Xsc, g->ldx, g->host_res_dev + 8, (size_t)0, (size_t)0,
                           (size_t)0, (const double*)nullptr, 0, 0, ++g->res_seq, (const double*)nullptr, 0, (size_t)0, (double*)nullptr,
                           (double*)nullptr);
        HIPCHK(hipGetLastError());
        {
            // (as in gp_finish: the kernel writes the Σ-vector, then this call's sequence number, into mapped host memory)
            volatile unsigned long long* seq = reinterpret_cast<volatile unsigned long long*>(g->host_res + 7);
            bool got = false;
            for (unsigned long i = 1;; ++i) {
                if (*seq == g->res_seq) {
                    got = true;
                    break;
                }
                if ((i & 0x3fff) == 0 && hipStreamQuery(s) != hipErrorNotReady) break;
            }
            std::atomic_thread_fence(std::memory_order_acquire);
            if (!got) HIPCHK(hipStreamSynchronize(s));
        }
        llgrad_finalize(d, g->N, g->host_par, g->host_par[d], g->host_par[d + 1], g->host_res[1], g->host_res + 8, grad_out);
        if (logpdf_out) *logpdf_out = loglik(g->N, g->host_res[0], g->host_res[1]);
        return BOSS_OK;
    }
    std::vector<double> h(nv);
    rc = llgrad_download(g, h);
    if (rc) return rc;
    // host_par still holds the staged parameters of the last update: 1/(λ+1e-8), (α+1e-8)², (σ+1e-8)²
    llgrad_finalize(d, g->N, g->host_par, g->host_par[d], g->host_par[d + 1], g->host_res[1], h.data(), grad_out);
    if (logpdf_out) *logpdf_out = loglik(g->N, g->host_res[0], g->host_res[1]);
    return BOSS_OK;
}

// boss_gp_loglike_grad plus ∂logpdf/∂mean_X[j] = (K⁻¹(y − m))_j — what carries the likelihood's gradient into the parameters of a
// Semiparametric model's mean (src/models/semiparametric.jl:79-92 under OptimizationMAP's AD, src/model_fitters/optimization.jl:146-164).
// Both paths keep a on the device anyway; here it comes back with the Σ-vector in one copy and one synchronisation.
extern "C" int boss_gp_loglike_grad_mean(boss_gp_t* g, double* logpdf_out, double* grad_out, double* dmean_out) {
    if (!g || !grad_out || !dmean_out) return fail(BOSS_E_INVALID, "NULL argument");
    NOT_FOR_MODELS(g);                                       // (the nonstationary model has boss_ngp_loglike_grad's dmean_out)
    KPROG_NEEDS_GRAD(g);
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = gp_settle(g);
    if (rc) return rc;
    const int d = g->d, nv = d + 2, N = g->N;
    if (d > LLG_MAX_D) return fail(BOSS_E_INVALID, "x_dim too large for the likelihood-gradient kernel");
    hipStream_t s = c->stream;
    std::vector<double> h((size_t)nv + N);
    if (small_fit_ok(c, N, d) && !g->kprog) {
        // N <= 128: the one-launch kernel, its results in device memory this time (N + d + 2 doubles, one copy back)
        rc = ws_reserve(c->pred, sizeof(double) * h.size());
        if (rc) return rc;
        double* sums = (double*)c->pred.p;
        dinv_join(g);
        hipLaunchKernelGGL(small_llgrad_kernel, dim3(1), dim3(DIAG_THREADS), SMALL_LLG_LDS_BYTES, s, (const double*)g->A, g->ld, g->Np, N, d,
                           g->kernel, g->amp2, (const double*)g->inv16, (const double*)g->Xsc, g->ldx, sums, (size_t)0, (size_t)0, (size_t)0,
                           (const double*)nullptr, 0, 0, 0ull, (const double*)nullptr, 0, (size_t)0, sums + nv, (double*)nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h.data(), sums, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } else {
        rc = llgrad_download(g, h, (size_t)N);
        if (rc) return rc;
    }
    llgrad_finalize(d, N, g->host_par, g->host_par[d], g->host_par[d + 1], g->host_res[1], h.data(), grad_out);
    std::copy(h.begin() + nv, h.end(), dmean_out);
    if (logpdf_out) *logpdf_out = loglik(N, g->host_res[0], g->host_res[1]);
    return BOSS_OK;
}

// data_loglike_slice of a NonstationaryGP (nonstationary_gp.jl:237-245) with its partial derivatives w.r.t. the latent models' values at
// the training points — what a fitter's AD carries back to the latent models through finite_nongp (:183-196).  Outputs (each may be
// NULL): dlam_out d×N (column j = ∂ℓ/∂λ(x_j), the layout of lam_X), damp_out N, dnoise_out N, dmean_out N.
extern "C" int boss_ngp_loglike_grad(boss_gp_t* g, double* logpdf_out, double* dlam_out, double* damp_out, double* dnoise_out,
                                     double* dmean_out) {
    if (!g) return fail(BOSS_E_INVALID, "gp is NULL");
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = gp_settle(g);
    if (rc) return rc;
    const int d = g->d, N = g->N, Np = g->Np;
    if (d > GIBBS_GRAD_MAX_D) return fail(BOSS_E_INVALID, "x_dim above 16 is not supported by the nonstationary gradient kernels");
    std::vector<double> h((size_t)(d + 3) * Np);
    rc = llgrad_download(g, h);
    if (rc) return rc;
    for (int j = 0; j < N; ++j) {
        if (dlam_out)
            for (int k = 0; k < d; ++k) dlam_out[(size_t)j * d + k] = h[(size_t)k * Np + j];
        if (damp_out) damp_out[j] = h[(size_t)d * Np + j];
        if (dnoise_out) dnoise_out[j] = h[(size_t)(d + 1) * Np + j];
        if (dmean_out) dmean_out[j] = h[(size_t)(d + 2) * Np + j];
    }
    if (logpdf_out) *logpdf_out = loglik(g->N, g->host_res[0], g->host_res[1]);
    return BOSS_OK;
}

// ∂ℓ/∂(λ_1..λ_d, α, σ, σ_∂) of the gradient-observation model from its d+3 sums h; hp = [1/(λ+1e-8) (d) | (α+1e-8)², (σ+1e-8)²,
// (σ_∂+1e-8)²], the staged parameters (a handle's host_par, a batch's parameter block)
static void ggp_llgrad_finalize(int d, const double* hp, const double* h, double* grad_out) {
    for (int m = 0; m < d; ++m) grad_out[m] = h[m];
    grad_out[d] = 2.0 * h[d] / std::sqrt(hp[d]);
    grad_out[d + 1] = std::sqrt(hp[d + 1]) * h[d + 1];
    grad_out[d + 2] = std::sqrt(hp[d + 2]) * h[d + 2];
}

// data_loglike of a GradientGaussianProcess and its gradient (gradient_gp.jl:367-397 under ForwardDiff, as OptimizationMAP takes it,
// src/model_fitters/optimization.jl:146-164): grad_out[d + 3] = ∂ℓ/∂(λ_1..λ_d, α, σ, σ_∂) at the parameters of the last boss_ggp_update.
extern "C" int boss_ggp_loglike_grad(boss_gp_t* g, double* logpdf_out, double* grad_out) {
    if (!g || !grad_out) return fail(BOSS_E_INVALID, "NULL argument");
    if (!g->aug) return fail(BOSS_E_INVALID, "handle was not created by boss_ggp_create");
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = gp_settle(g);
    if (rc) return rc;
    const int d = g->d, nv = d + 3;
    if (d > AUG_MAX_D) return fail(BOSS_E_INVALID, "x_dim too large for the gradient-observation kernels");
    std::vector<double> h(nv);
    rc = llgrad_download(g, h);
    if (rc) return rc;
    ggp_llgrad_finalize(d, g->host_par, h.data(), grad_out);   // (host_par: the staged parameters of the last update)
    if (logpdf_out) *logpdf_out = loglik(g->N, g->host_res[0], g->host_res[1]);
    return BOSS_OK;
}
