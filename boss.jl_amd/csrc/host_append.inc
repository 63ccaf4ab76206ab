// host_append.inc — growing a handle, block Cholesky append, rank-one append on resident inverses (included by bosship.hip).

// ------------------------------------------------------------------------------------------
// block Cholesky append (SURVEY §8f2): augment_dataset! + model_posterior with unchanged
// hyper-parameters.  Only the block rows that contain new observations are (re)built: their
// Gram rows are swept through the finished panels 0..kb-1 (solve with L_kk, rank-128 update of
// the rest of the block row and of its δ^T entries), then the diagonal block is factorised like
// any other — the right-looking factorisation restricted to one block row, O(N²) per 128 rows.
// ------------------------------------------------------------------------------------------
// A member of a batch-fitted set (boss_gp_fit_batch) shares its observations with its siblings and lives in their slab: before
// anything rewrites the data or re-lays the arrays out, it gets arrays of its own (same sizes, contents copied) and leaves the set.
// Caller holds the context lock; no update is pending.
static int gp_own(boss_gp* g) {
    if (!g->set) return BOSS_OK;
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    const size_t Np = g->Np, d = g->d, ldx = g->ldx;          // (ldx: Np, or the padded point count of a gradient-observation member)
    constexpr int NA = 13;                                   // the last three: λ(X), α(X), σ(X) of a nonstationary member
    double* nw[NA] = {};
    double* src[NA] = {g->Xraw, g->Xsc, g->y, g->mean, g->A, g->inv16, g->Dinv, g->Dinv2, g->invlam, g->scal, g->lamX, g->ampX, g->noiseX};
    const size_t bytes[NA] = {sizeof(double) * d * ldx, sizeof(double) * d * ldx, sizeof(double) * Np, sizeof(double) * Np,
                              sizeof(double) * (size_t)g->ld * Np, sizeof(double) * g->nblk * 8 * 256, sizeof(double) * g->nblk * BLK * BLK,
                              sizeof(double) * Np * PRED_RB, sizeof(double) * (d + 4), sizeof(double) * 4,
                              g->gibbs ? sizeof(double) * d * Np : 0, g->gibbs ? sizeof(double) * Np : 0, g->gibbs ? sizeof(double) * Np : 0};
    double *hres = nullptr, *hpar = nullptr, *hres_dev = nullptr;
    bool ok = true;
    for (int i = 0; i < NA && ok; ++i) ok = bytes[i] == 0 || dev_malloc((void**)&nw[i], bytes[i]) == hipSuccess;
    ok = ok && hipHostMalloc((void**)&hres, 512, hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc((void**)&hpar, sizeof(double) * (d + 4), hipHostMallocDefault) == hipSuccess &&
         hipHostGetDevicePointer((void**)&hres_dev, hres, 0) == hipSuccess;
    dinv_join(g);
    hipError_t e = hipSuccess;
    for (int i = 0; i < NA && ok && e == hipSuccess; ++i)
        if (bytes[i]) e = hipMemcpyAsync(nw[i], src[i], bytes[i], hipMemcpyDeviceToDevice, s);
    if (ok && e == hipSuccess) e = hipStreamSynchronize(s);
    if (!ok || e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        for (double* p : nw)
            if (p) (void)hipFree(p);
        if (hres) (void)hipHostFree(hres);
        if (hpar) (void)hipHostFree(hpar);
        return ok ? fail(BOSS_E_NO_DEVICE, std::string("detaching a posterior from its batch: ") + hipGetErrorString(e))
                  : fail(BOSS_E_ALLOC, "device allocation failed while detaching a posterior from its batch");
    }
    std::memcpy(hres, g->host_res, 512);
    std::memcpy(hpar, g->host_par, sizeof(double) * (d + 4));
    boss_gpset* st = g->set;
    if (st->refs.fetch_sub(1) == 1) {
        if (st->slab) (void)hipFree(st->slab);
        if (st->host_block) (void)hipHostFree(st->host_block);
        delete st;
    }
    g->set = nullptr;
    g->Xraw = nw[0]; g->Xsc = nw[1]; g->y = nw[2]; g->mean = nw[3]; g->A = nw[4]; g->inv16 = nw[5]; g->Dinv = nw[6]; g->Dinv2 = nw[7];
    g->invlam = nw[8];
    g->hyp = g->invlam + d;
    g->scal = nw[9];
    g->info = (int*)(g->scal + 2);
    g->lamX = nw[10]; g->ampX = nw[11]; g->noiseX = nw[12];
    g->host_res = hres;
    g->host_res_dev = hres_dev;
    g->host_par = hpar;
    return BOSS_OK;
}

static int gp_grow(boss_gp* g, int Nnew) {
    if (Nnew > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");
    {
        int rc = gp_own(g);                                  // (a member of a batch-fitted set first gets arrays of its own)
        if (rc) return rc;
    }
    const int Np2 = round_up(Nnew, PRED_RB);
    if (Np2 <= g->Np) return BOSS_OK;
    chain_quiesce(g->ctx);                                   // (the arrays are about to be replaced)
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    const int Np = g->Np, d = g->d, nblk2 = Np2 / BLK, ld2 = Np2 + RHS_ROWS;
    // (a gradient-observation handle keeps its points at a pitch of their own, which ggp_grow_points grows: copied as they are)
    const int ldx1 = g->aug ? g->ldx : Np, ldx2 = g->aug ? g->ldx : Np2;
    const size_t szA = sizeof(double) * (size_t)ld2 * Np2;
    double* nw[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[8] = {sizeof(double) * d * ldx2, sizeof(double) * d * ldx2, sizeof(double) * Np2, sizeof(double) * Np2,
                             szA, sizeof(double) * nblk2 * 8 * 256, sizeof(double) * nblk2 * BLK * BLK,
                             sizeof(double) * (size_t)Np2 * PRED_RB};
    for (int i = 0; i < 8; ++i)
        if (dev_malloc((void**)&nw[i], bytes[i]) != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipFree(nw[j]);
            return fail(BOSS_E_ALLOC, "device allocation failed while growing the posterior handle");
        }
    // a nonstationary handle: λ(X) [d][Np2], α(X), σ(X) [Np2]; padded like boss_ngp_update pads them (λ = 1, α = σ = 0)
    double* nlat[3] = {nullptr, nullptr, nullptr};
    const size_t lbytes[3] = {sizeof(double) * d * Np2, sizeof(double) * Np2, sizeof(double) * Np2};
    if (g->gibbs)
        for (int i = 0; i < 3; ++i)
            if (dev_malloc((void**)&nlat[i], lbytes[i]) != hipSuccess) {
                for (int j = 0; j < 8; ++j) (void)hipFree(nw[j]);
                for (int j = 0; j < i; ++j) (void)hipFree(nlat[j]);
                return fail(BOSS_E_ALLOC, "device allocation failed while growing the posterior handle");
            }
    hipError_t e = hipSuccess;
    for (int i = 0; i < 5 && e == hipSuccess; ++i) e = hipMemsetAsync(nw[i], 0, bytes[i], s);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(nw[0], sizeof(double) * ldx2, g->Xraw, sizeof(double) * ldx1, sizeof(double) * ldx1, d,
                             hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(nw[1], sizeof(double) * ldx2, g->Xsc, sizeof(double) * ldx1, sizeof(double) * ldx1, d,
                             hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nw[2], g->y, sizeof(double) * Np, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nw[3], g->mean, sizeof(double) * Np, hipMemcpyDeviceToDevice, s);
    // factor: rows 0..Np-1 of every old column; the δ^T / z row block moves from row Np to row Np2
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(nw[4], sizeof(double) * ld2, g->A, sizeof(double) * g->ld, sizeof(double) * Np, Np,
                             hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(nw[4] + Np2, sizeof(double) * ld2, g->A + Np, sizeof(double) * g->ld,
                             sizeof(double) * RHS_ROWS, Np, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(nw[5], g->inv16, sizeof(double) * g->nblk * 8 * 256, hipMemcpyDeviceToDevice, s);
    if (g->gibbs) {
        const size_t nl = (size_t)d * Np2;
        hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s, nlat[0], 1.0, nl);
        for (int i = 1; i < 3 && e == hipSuccess; ++i) e = hipMemsetAsync(nlat[i], 0, lbytes[i], s);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(nlat[0], sizeof(double) * Np2, g->lamX, sizeof(double) * Np, sizeof(double) * Np, d,
                                 hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nlat[1], g->ampX, sizeof(double) * Np, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nlat[2], g->noiseX, sizeof(double) * Np, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipGetLastError();
    }
    dinv_join(g);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {                                   // the handle keeps its old arrays; the new ones go back
        (void)hipStreamSynchronize(s);
        for (int i = 0; i < 8; ++i) (void)hipFree(nw[i]);
        for (double* p : nlat)
            if (p) (void)hipFree(p);
        return fail(BOSS_E_NO_DEVICE, std::string("growing the posterior handle: ") + hipGetErrorString(e));
    }
    if (g->gibbs) {
        double* oldlat[3] = {g->lamX, g->ampX, g->noiseX};
        for (double* p : oldlat) (void)hipFree(p);
        g->lamX = nlat[0]; g->ampX = nlat[1]; g->noiseX = nlat[2];
    }
    double* old[8] = {g->Xraw, g->Xsc, g->y, g->mean, g->A, g->inv16, g->Dinv, g->Dinv2};
    for (double* p : old) (void)hipFree(p);
    if (g->LT) (void)hipFree(g->LT);
    if (g->DT2) (void)hipFree(g->DT2);
    if (g->avec) (void)hipFree(g->avec);
    g->LT = g->DT2 = g->avec = nullptr;
    if (g->Winv) (void)hipFree(g->Winv);
    if (g->Linv) (void)hipFree(g->Linv);
    g->Winv = g->Linv = nullptr;
    if (g->W2) (void)hipFree(g->W2);
    g->W2 = nullptr;
    g->Xraw = nw[0]; g->Xsc = nw[1]; g->y = nw[2]; g->mean = nw[3]; g->A = nw[4]; g->inv16 = nw[5]; g->Dinv = nw[6]; g->Dinv2 = nw[7];
    g->Np = Np2;
    g->nblk = nblk2;
    g->ld = ld2;
    ++g->factor_gen;
    g->have_dinv = false;
    g->have_winv = false;
    g->few_calls = 0;
    g->have_lt = false;
    return BOSS_OK;
}

// Reserve storage for observations that will be appended later (no re-allocation / re-layout when
// they arrive).  The extra rows are identity padding of the factor: harmless, a little extra work per
// factorisation.  The handle is left unfitted: call boss_gp_update afterwards.
static int reserve_locked_entry(boss_gp* g, int N_total);
extern "C" int boss_gp_reserve(boss_gp_t* g, int N_total) {
    if (!g || N_total < 1) return fail(BOSS_E_INVALID, "bad arguments");
    NOT_FOR_MODELS(g);
    KPROG_NEEDS_SEQ(g);
    return reserve_locked_entry(g, N_total);
}
// The same for a nonstationary handle: λ(X), α(X), σ(X) grow with the rest (gp_grow); follow with boss_ngp_update, whose latent
// arrays still have N columns — the reserved columns are padding.
extern "C" int boss_ngp_reserve(boss_gp_t* g, int N_total) {
    if (!g || N_total < 1) return fail(BOSS_E_INVALID, "bad arguments");
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    return reserve_locked_entry(g, N_total);
}
// The points of a gradient-observation handle, Xraw / Xsc [d][ldx]: their pitch grows in steps of 64 points (the Gram and K*
// kernels read whole 64-point groups).  Caller holds the context lock; the handle owns its arrays (gp_own).
static int ggp_grow_points(boss_gp* g, int npts_new) {
    const int ldx2 = round_up(npts_new, 64);
    if (ldx2 <= g->ldx) return BOSS_OK;
    hipStream_t s = g->ctx->stream;
    const int d = g->d, ldx = g->ldx;
    const size_t bytes = sizeof(double) * d * ldx2;
    double* nw[2] = {nullptr, nullptr};
    if (dev_malloc((void**)&nw[0], bytes) != hipSuccess || dev_malloc((void**)&nw[1], bytes) != hipSuccess) {
        if (nw[0]) (void)hipFree(nw[0]);
        return fail(BOSS_E_ALLOC, "device allocation failed while growing the posterior handle");
    }
    double* old[2] = {g->Xraw, g->Xsc};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipMemsetAsync(nw[i], 0, bytes, s);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(nw[i], sizeof(double) * ldx2, old[i], sizeof(double) * ldx, sizeof(double) * ldx, d, hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {                                   // the handle keeps its old arrays
        (void)hipStreamSynchronize(s);
        (void)hipFree(nw[0]);
        (void)hipFree(nw[1]);
        return fail(BOSS_E_NO_DEVICE, std::string("growing the posterior handle: ") + hipGetErrorString(e));
    }
    (void)hipFree(old[0]);
    (void)hipFree(old[1]);
    g->Xraw = nw[0];
    g->Xsc = nw[1];
    g->ldx = ldx2;
    return BOSS_OK;
}

// The same for a gradient-observation handle, counted in POINTS: n_points_total (1 + d) rows and the points' own pitch; follow with
// boss_ggp_update.
extern "C" int boss_ggp_reserve(boss_gp_t* g, int n_points_total) {
    if (!g || n_points_total < 1) return fail(BOSS_E_INVALID, "bad arguments");
    if (!g->aug) return fail(BOSS_E_INVALID, "handle was not created by boss_ggp_create");
    if ((long long)n_points_total * (1 + g->d) > MAX_ROWS) return fail(BOSS_E_INVALID, "augmented system too large (n (1 + d) > 46080)");
    return reserve_locked_entry(g, n_points_total * (1 + g->d));
}
static int reserve_locked_entry(boss_gp* g, int N_total) {
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    if (g->pending) (void)gp_finish(g, nullptr);
    int rc = gp_grow(g, N_total);
    if (rc) return rc;
    if (g->aug) {
        rc = ggp_grow_points(g, N_total / (1 + g->d));
        if (rc) return rc;
    }
    g->fitted = false;
    ++g->epoch;
    g->append_calls = 0;
    return BOSS_OK;
}

// Knobs the rank-one append shares with the few-candidate prediction (host_predict.inc).  BOSS_WINV_AFTER: the call with few
// candidates on one factorisation from which on the inverse factors are built and kept resident (0: never).  BOSS_NO_FEW_ARGS=1:
// points and candidates go through device buffers, never through kernel arguments.
static int winv_after() {
    static const int v = getenv("BOSS_WINV_AFTER") ? atoi(getenv("BOSS_WINV_AFTER")) : 2;
    return v;
}
static bool few_args_off() {
    static const bool v = getenv("BOSS_NO_FEW_ARGS") && atoi(getenv("BOSS_NO_FEW_ARGS"));
    return v;
}

// A pending update is finished and the handle must be fitted (gp_settle); a posterior with a prior mean needs its values at the
// new points.  Caller holds the context lock.
static int append_settle(boss_gp* g, const char* unfitted, const double* mean_new) {
    int rc = gp_settle(g, unfitted);
    if (rc) return rc;
    if (g->has_mean && !mean_new)
        return fail(BOSS_E_INVALID, "the posterior has a prior mean: mean_new (its values at the new points) is required");
    return BOSS_OK;
}

// The n new points (rounded where discrete) behind the resident ones, the ny new rows of y and, where given, of the prior mean
// behind row N; waits for the copies, so the caller's and the staging buffers may go.  Caller holds the context lock; the handle
// has room (gp_grow) and still counts the old observations.
static int append_upload(boss_gp* g, int n, const double* X_new, int ny, const double* y_rows, const double* mean_new) {
    hipStream_t s = g->ctx->stream;
    const int d = g->d, N0 = g->N;
    const int col0 = g->aug ? g->npts : N0, pitch = g->aug ? g->ldx : g->Np;   // (a gradient-observation handle: one column per POINT)
    std::vector<double> xb;
    pack_points(xb, X_new, d, n, n, g->discrete.empty() ? nullptr : g->discrete.data());
    HIPCHK(hipMemcpy2DAsync(g->Xraw + col0, sizeof(double) * pitch, xb.data(), sizeof(double) * n, sizeof(double) * n, d,
                            hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->y + N0, y_rows, sizeof(double) * ny, hipMemcpyHostToDevice, s));
    if (mean_new) {
        HIPCHK(hipMemcpyAsync(g->mean + N0, mean_new, sizeof(double) * ny, hipMemcpyHostToDevice, s));
        g->has_mean = true;
    }
    HIPCHK(hipStreamSynchronize(s));           // staging buffers go out of scope
    return BOSS_OK;
}

// The block rows N0 … N1 − 1 of the factor, for every model: those holding new observations and, when the storage has just grown
// (Np_before != Np), the pure padding block rows behind them as well (identity blocks of the factor and their inverses: the new
// arrays are uninitialised).  Each block row's Gram tiles — from the model's own Gram kernel — are swept through the finished
// panels, then its diagonal block is factorised; where most of the matrix is new, a plain re-factorisation is cheaper than
// block-row sweeps.  Ends with the results on their way to host_res: follow with update_finish.  Caller holds the context lock;
// the data of the new rows is resident and g->N counts them.
static int append_rows_enqueue(boss_gp* g, int N0, int N1, int Np_before) {
    hipStream_t s = g->ctx->stream;
    const int kb0 = N0 / BLK, kb1 = (g->Np != Np_before) ? g->nblk - 1 : (N1 - 1) / BLK;
    if (kb1 - kb0 + 1 > 4 || kb1 - kb0 + 1 >= g->nblk) {
        g->append_path = 2;
        return factor_enqueue(g);
    }
    g->append_path = 1;
    const int d = g->d, Np = g->Np, ld = g->ld;
    dinv_join(g);
    HIPCHK(hipMemsetAsync(g->info, 0, sizeof(int), s));
    if (!g->aug && !g->gibbs)
        hipLaunchKernelGGL(scale_points_kernel, dim3((Np + 255) / 256, 1, 1), dim3(256), 0, s, g->Xraw, g->Xsc, (size_t)0,
                           g->invlam, d, Np);
    for (int kb = kb0; kb <= kb1; ++kb) {
        hipLaunchKernelGGL(rhs_rows_kernel, dim3(1, 1, 1), dim3(BLK), 0, s, g->A, ld, (size_t)0, N1, Np, g->y, g->mean,
                           (size_t)0, kb * BLK, (int*)nullptr);
        // 128 rows × columns 0 … (kb+1)·128 − 1: the 4·kb + 3 tiles from triangular tile index kb (2 kb + 1), a full build's arithmetic
        const dim3 tiles(4 * kb + 3, 1, 1);
        const int tile0 = kb * (2 * kb + 1);
        if (g->aug)
            hipLaunchKernelGGL(aug_gram_kernel, tiles, dim3(256), 0, s, (const double*)g->Xraw, g->ldx, d, g->nhead, N1,
                               Np, g->kernel, (const double*)g->hyp, (const double*)g->invlam, (size_t)0, g->A, ld, (size_t)0, tile0);
        else if (g->gibbs)
            hipLaunchKernelGGL(gibbs_gram_kernel, tiles, dim3(256), 0, s, (const double*)g->Xraw,
                               (const double*)g->lamX, (const double*)g->ampX, (const double*)g->noiseX, (size_t)0, (size_t)0, d, N1,
                               Np, g->A, ld, (size_t)0, tile0);
        else if (g->kprog)
            kprog_gram_rows_launch(g, kb, s);                // (the same tiles under the program: N1 = g->N bounds the valid rows)
        else
            hipLaunchKernelGGL(gram_kernel, tiles, dim3(256), 0, s, g->Xsc, (size_t)0, d, N1, Np, g->kernel,
                               g->hyp, g->A, ld, (size_t)0, tile0);
        for (int k = 0; k < kb; ++k) {
            hipLaunchKernelGGL(potrf_trsm_kernel, dim3(8, 1, 1), dim3(TRSM_THREADS), 0, s, g->A, ld, (size_t)0, k, g->inv16, (size_t)0,
                               kb * BLK);
            hipLaunchKernelGGL(potrf_rowupd_kernel, dim3(4 * (kb - k) + 1), dim3(256), 0, s, g->A, ld, k, kb, Np);
        }
        hipLaunchKernelGGL(potrf_diag_kernel, dim3(1, 1, 1), dim3(DIAG_THREADS), DIAG_LDS_BYTES, s, g->A, ld, (size_t)0, kb,
                           g->inv16, (size_t)0, g->info, (unsigned long long*)nullptr, 0ull);
        hipLaunchKernelGGL(potrf_trsm_kernel, dim3(1, 1, 1), dim3(TRSM_THREADS), 0, s, g->A, ld, (size_t)0, kb, g->inv16, (size_t)0,
                           Np);
    }
    dinv_eager(g);
    hipLaunchKernelGGL(potrf_logdet_kernel, dim3(1, 1, 1), dim3(LOGDET_THREADS), 0, s, g->A, ld, (size_t)0, N1, Np, g->scal,
                       (double*)nullptr, (const int*)nullptr, (unsigned long long*)nullptr, 0ull, 0ull);
    HIPCHK(hipMemcpyAsync(g->host_res, g->scal, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&g->host_res[2], g->info, sizeof(int), hipMemcpyDeviceToHost, s));
    return BOSS_OK;
}

static int append_locked(boss_gp* g, int n, const double* X_new, const double* y_new, const double* mean_new, double* logpdf_out);

extern "C" int boss_gp_append(boss_gp_t* g, int n, const double* X_new, const double* y_new, const double* mean_new,
                              double* logpdf_out) {
    if (!g || n < 1 || !X_new || !y_new) return fail(BOSS_E_INVALID, "need a handle, n >= 1 and non-NULL X_new, y_new");
    NOT_FOR_MODELS(g);
    KPROG_NEEDS_SEQ(g);
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    if (n > 1 && n <= 8 && g->have_winv && g->fitted && !g->pending && g->N + n <= g->Np) {
        // a handful of observations on resident inverse factors: n rank-one appends beat one block-row sweep
        // (a failure part-way leaves the observations appended so far in the handle: boss_gp_n tells the caller how many)
        int rc = BOSS_OK;
        for (int j = 0; j < n && rc == BOSS_OK; ++j)
            rc = append_locked(g, 1, X_new + (size_t)j * g->d, y_new + j, mean_new ? mean_new + j : nullptr, logpdf_out);
        return rc;
    }
    return append_locked(g, n, X_new, y_new, mean_new, logpdf_out);
}

// caller holds the context lock
static int append_locked(boss_gp* g, int n, const double* X_new, const double* y_new, const double* mean_new, double* logpdf_out) {
    Ctx* c = g->ctx;
    int rc = append_settle(g, "append needs a fitted handle (its hyper-parameters are reused)", mean_new);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const int d = g->d, N0 = g->N, N1 = N0 + n;
    const int Np_before = g->Np;
    // one observation into existing storage, not the first such append on these hyper-parameters: rank-one append on the
    // resident inverse factors (built here if they are not resident yet)
    bool fast = false;
    if (n == 1 && N1 <= g->Np && winv_after() > 0 && sizeof(double) * (size_t)g->Np <= 144 * 1024) {
        if (!g->have_winv && ++g->append_calls >= 2 && g->few_calls >= 0) {
            const size_t bytes = sizeof(double) * (size_t)g->ld * g->Np;
            bool ok = (g->Winv != nullptr || dev_malloc((void**)&g->Winv, bytes) == hipSuccess) &&
                      (g->Linv != nullptr || dev_malloc((void**)&g->Linv, bytes) == hipSuccess);
            if (ok) {
                dinv_join(g);
                if (!g->have_dinv) {
                    dinv_launch(g, s);
                    g->have_dinv = true;
                }
                linv_enqueue(g, s, g->Winv, g->Linv);
                g->have_winv = true;
            } else {
                (void)hipGetLastError();
                g->few_calls = -(1 << 30);
            }
        }
        fast = g->have_winv;
    }
    rc = gp_grow(g, N1);
    if (rc) return rc;
    gp_invalidate_append(g, fast);
    // one observation on resident inverse factors, x_dim small enough for kernel arguments: no upload, no synchronisation in front
    // (a program kernel takes the device-buffer variant: its K* needs the interpreter, which the kernel-argument and fused variants
    // do not carry — a later optimisation)
    const bool by_args = fast && n == 1 && d <= FEW_ARGS_MAX_D && !few_args_off() && !g->kprog;
    if (!by_args) {
        rc = append_upload(g, n, X_new, n, y_new, mean_new);
        if (rc) return rc;
    }
    g->N = N1;
    if (fast) {
        g->append_path = 3;
        const int Np = g->Np, ld = g->ld, nwg = Np / WINV_ROWS;
        dinv_join(g);
        if (!g->have_dinv) {                                 // the patched blocks must exist
            dinv_launch(g, s);
            g->have_dinv = true;
        }
        rc = ws_reserve(c->few, sizeof(double) * ((size_t)Np * 32 + (size_t)nwg * 8 + 2 * (size_t)Np + 8));
        if (rc) return rc;
        rc = ws_reserve(c->csc, sizeof(double) * (size_t)d * 64);
        if (rc) return rc;
        double* R = (double*)c->few.p;                       // k = K(X, x_new) in column 0 of a 32-wide tile
        double* part = R + (size_t)Np * 32;
        double* lvec = part + (size_t)nwg * 8;
        double* wvec = lvec + Np;
        double* dz = wvec + Np;
        double* kself = g->kprog ? dz + 2 : nullptr;         // program kernel: k(x_new, x_new), evaluated (no constant prior variance)
        double* Csc = (double*)c->csc.p;
        bool fused_done = false;
        if (by_args) {
            AppendPoint ap;
            FewCand fc;
            ap.d = d;
            ap.N0 = N0;
            ap.Np = Np;
            ap.y = y_new[0];
            ap.mean = mean_new ? mean_new[0] : 0.0;
            fc.ncols = 1;
            for (int j = 0; j < WINV_MAX_M; ++j) {
                fc.mean[j] = 0.0;
                for (int k = 0; k < FEW_ARGS_MAX_D; ++k) fc.x[j][k] = 0.0;
            }
            for (int k = 0; k < FEW_ARGS_MAX_D; ++k) {
                double v = k < d ? X_new[k] : 0.0;
                if (k < d && !g->discrete.empty() && g->discrete[k]) v = std::nearbyint(v);   // kernels.jl:56-59
                ap.raw[k] = v;
                ap.sc[k] = k < d ? v * g->host_par[k] : 0.0;                                    // 1/(λ + 1e-8) of the last update
                fc.x[0][k] = ap.sc[k];
            }
            if (mean_new) g->has_mean = true;
            const bool fused = few_fused() && few_done_ensure(c, s) && sizeof(double) * (size_t)Np <= 144 * 1024;
            if (fused) {
                // critical path to the caller's answer: K*, then ONE launch for the pass over L⁻ᵀ and the scalars (small_calls.hpp); the new
                // point's rows are written behind it (nothing before reads them: its value and mean travel in the arguments too)
                hipLaunchKernelGGL(kstar_args_kernel, dim3(Np / 256), dim3(256), 0, s, fc, (const double*)g->Xsc, Np, N0, d, g->kernel, g->amp2, R, 1);
                AppendTail tail;
                tail.y = ap.y;
                tail.mean = ap.mean;
                tail.N0 = N0;
                tail.hyp = g->hyp;
                tail.scal = g->scal;
                tail.dz = dz;
                tail.vout = lvec;
                tail.info = g->info;
                c->few_done_cnt += (unsigned long long)nwg;
                const size_t lds = sizeof(double) * std::max((size_t)Np, (size_t)(8 * 256 + 64));
                hipLaunchKernelGGL((winv_args_kernel<1, true>), dim3(nwg), dim3(256), lds, s, fc, (const double*)g->Xsc, N0, d, g->kernel, g->amp2,
                                   (const double*)g->Winv, ld, Np, (const double*)g->A, ld, (const double*)R, part, c->few_done, c->few_done_cnt,
                                   g->host_res_dev, ++g->res_seq, tail);
                hipLaunchKernelGGL(append_point_kernel, dim3(1), dim3(64), 0, s, ap, g->Xraw, g->Xsc, g->y, g->mean, (int*)nullptr);
                fused_done = true;
            } else {
                hipLaunchKernelGGL(append_point_kernel, dim3(1), dim3(64), 0, s, ap, g->Xraw, g->Xsc, g->y, g->mean, g->info);
                hipLaunchKernelGGL(kstar_args_kernel, dim3(Np / 256), dim3(256), 0, s, fc, (const double*)g->Xsc, Np, N0, d, g->kernel, g->amp2, R);
            }
        } else {
            HIPCHK(hipMemsetAsync(g->info, 0, sizeof(int), s));
            hipLaunchKernelGGL(scale_points_kernel, dim3((Np + 255) / 256, 1, 1), dim3(256), 0, s, g->Xraw, g->Xsc, (size_t)0, g->invlam, d, Np);
            // the new (scaled) point as candidate 0 of a 64-wide candidate block
            HIPCHK(hipMemcpy2DAsync(Csc, sizeof(double) * 64, g->Xsc + N0, sizeof(double) * Np, sizeof(double), d, hipMemcpyDeviceToDevice, s));
            if (g->kprog)
                kprog_append_col_launch(g, N0, Csc, R, kself, s);
            else
                hipLaunchKernelGGL(kstar_rows_kernel, dim3(Np / 256, 1), dim3(256), sizeof(double) * (d * 32 + KSTAR_LDS_EXTRA), s, (const double*)g->Xsc, Np, N0,
                                   (const double*)Csc, d, 64, g->kernel, g->amp2, R, 1);
        }
        if (!fused_done) {
            hipLaunchKernelGGL(winv_gemv_kernel<1>, dim3(nwg), dim3(256), sizeof(double) * (size_t)Np, s, (const double*)g->Winv, ld, Np,
                               (const double*)g->A, ld, (const double*)R, 1, part, lvec);
            // (by_args: the scalars kernel hands {logdet, zᵀz, info} to the host itself — the call returns while the second pass runs)
            hipLaunchKernelGGL(append_scalars_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nwg, (const double*)g->hyp,
                               (const double*)g->y, (const double*)g->mean, N0, g->scal, dz, g->info, by_args ? g->host_res_dev : (double*)nullptr,
                               by_args ? ++g->res_seq : 0ull, (const double*)kself);
        }
        hipLaunchKernelGGL(linv_col_gemv_kernel, dim3((N0 + 7) / 8), dim3(256), 0, s, (const double*)g->Linv, ld, N0,
                           (const double*)lvec, wvec);
        hipLaunchKernelGGL(append_write_kernel, dim3(N0 / 256 + 1), dim3(256), 0, s, g->A, ld, Np, N0, (const double*)lvec,
                           (const double*)wvec, (const double*)dz, g->Linv, g->Winv, g->Dinv, g->Dinv2, g->inv16);
        if (by_args) {
            g->res_polled = true;
        } else {
            HIPCHK(hipMemcpyAsync(g->host_res, g->scal, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(&g->host_res[2], g->info, sizeof(int), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipGetLastError());
        g->pending = true;
        rc = gp_finish(g, logpdf_out);
        if (rc) {                                            // not positive definite: nothing resident describes the data any more
            g->have_dinv = false;
            g->have_winv = false;
        }
        return rc;
    }
    rc = append_rows_enqueue(g, N0, N1, Np_before);
    if (rc) return rc;
    return update_finish(g, 0, logpdf_out);
}

// augment_dataset! (src/types/problem.jl:191-198) + the posterior of a nonstationary model with the latent models evaluated by
// the caller AT THE NEW POINTS only.  k(x_i, x_j) depends on λ, α at x_i and x_j alone, and those of the old points stay resident
// (lamX, ampX, noiseX): no entry between two old points changes, the new observations go to the end of the ordering, so the
// leading block of the factor stays valid exactly as for a stationary kernel — the block rows that hold new observations are
// rebuilt (append_rows_enqueue, the Gram tiles from gibbs_gram_kernel), or the grown arrays are factorised again on the device
// where most of the matrix is new.  Nothing of the handle's data travels to the host.
extern "C" int boss_ngp_append(boss_gp_t* g, int n_new, const double* X_new, const double* y_new, const double* lam_new,
                               const double* amp_new, const double* noise_new, const double* mean_new, double* logpdf_out) {
    if (!g || n_new < 1 || !X_new || !y_new || !lam_new || !amp_new || !noise_new) return fail(BOSS_E_INVALID, "NULL argument or n_new < 1");
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    Ctx* c = g->ctx;
    const int d = g->d, n = n_new;
    std::vector<double> lb((size_t)d * n);                  // λ at the new points, [d][n] like lamX
    for (int j = 0; j < n; ++j) {
        for (int k = 0; k < d; ++k) {
            const double v = lam_new[(size_t)j * d + k];
            if (!(v > 0.0) || !std::isfinite(v)) return fail(BOSS_E_INVALID, "lengthscales must be finite and > 0");
            lb[(size_t)k * n + j] = v;
        }
        if (!(amp_new[j] >= 0.0) || !std::isfinite(amp_new[j])) return fail(BOSS_E_INVALID, "amplitudes must be finite and >= 0");
        if (!(noise_new[j] >= 0.0) || !std::isfinite(noise_new[j])) return fail(BOSS_E_INVALID, "noise stds must be finite and >= 0");
    }
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = append_settle(g, "handle has no valid factorisation (its per-point hyper-parameters are the ones re-used)", mean_new);
    if (rc) return rc;
    if ((long long)g->N + n > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");
    hipStream_t s = c->stream;
    const int N0 = g->N, N1 = N0 + n;
    const int Np_before = g->Np;
    rc = gp_grow(g, N1);
    if (rc) return rc;
    gp_invalidate_append(g, false);
    const size_t pitch = sizeof(double) * g->Np, row = sizeof(double) * n;
    HIPCHK(hipMemcpy2DAsync(g->lamX + N0, pitch, lb.data(), row, row, d, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->ampX + N0, amp_new, row, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->noiseX + N0, noise_new, row, hipMemcpyHostToDevice, s));
    rc = append_upload(g, n, X_new, n, y_new, mean_new);     // (waits for the three copies above as well)
    if (rc) return rc;
    g->N = N1;
    rc = append_rows_enqueue(g, N0, N1, Np_before);
    if (rc) return rc;
    return update_finish(g, 0, logpdf_out);
}

// augment_dataset! (src/types/problem.jl:191-198) followed by the posterior at unchanged hyper-parameters for a gradient-observation
// model.  X_new d×n_new, y_new n_new, dY_new d×n_new column-major.  The reference's ordering [y; ∂_1 y; …; ∂_d y] would put new rows
// inside every block; the handle's own ordering (aug_row_decode, gram_kernels.hpp) puts the 1 + d rows of every appended point at
// the end instead, a symmetric permutation the posterior does not see.  The leading block of the factor then survives, and the
// append runs as the other models' does: the block rows that hold new rows are rebuilt (append_rows_enqueue, the Gram tiles
// from aug_gram_kernel), or the grown arrays are factorised again on the device where most of the matrix is new.
// Nothing of the handle's data travels to the host and the hyper-parameters staged on the device by the last update are the ones
// used, verbatim.
extern "C" int boss_ggp_append(boss_gp_t* g, int n_new, const double* X_new, const double* y_new, const double* dY_new, double* logpdf_out) {
    if (!g || !X_new || !y_new || !dY_new || n_new < 1) return fail(BOSS_E_INVALID, "need a handle, n_new >= 1 and non-NULL X_new, y_new, dY_new");
    if (!g->aug) return fail(BOSS_E_INVALID, "handle was not created by boss_ggp_create");
    Ctx* c = g->ctx;
    const int d = g->d, n = n_new;
    if ((long long)(g->npts + n) * (1 + d) > MAX_ROWS) return fail(BOSS_E_INVALID, "augmented system too large (n (1 + d) > 46080)");
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    int rc = gp_settle(g, "handle has no valid factorisation (its hyper-parameters are the ones re-used)");
    if (rc) return rc;
    const int N0 = g->N, N1 = N0 + n * (1 + d), n0 = g->npts;
    const int Np_before = g->Np;
    rc = gp_grow(g, N1);                                     // (a member of a batch-fitted set leaves it here: gp_own)
    if (rc) return rc;
    rc = ggp_grow_points(g, n0 + n);
    if (rc) return rc;
    gp_invalidate_append(g, false);
    std::vector<double> yb((size_t)n * (1 + d));
    for (int j = 0; j < n; ++j) {                            // the rows of an appended point: [y_j, ∂y_j/∂x_1 … ∂y_j/∂x_d]
        yb[(size_t)j * (1 + d)] = y_new[j];
        for (int l = 0; l < d; ++l) yb[(size_t)j * (1 + d) + 1 + l] = dY_new[(size_t)j * d + l];
    }
    rc = append_upload(g, n, X_new, (int)yb.size(), yb.data(), nullptr);
    if (rc) return rc;
    g->N = N1;
    g->npts = n0 + n;
    rc = append_rows_enqueue(g, N0, N1, Np_before);
    if (rc) return rc;
    return update_finish(g, 0, logpdf_out);
}

// How the handle's last append ran (tests): 0 no append yet, 1 block rows, 2 full re-factorisation on the device, 3 rank-one on
// resident inverses.  No device work.
extern "C" int boss_debug_append_path(const boss_gp_t* g, int* path_out) {
    if (!g || !path_out) return fail(BOSS_E_INVALID, "bad argument");
    *path_out = g->append_path;
    return BOSS_OK;
}

extern "C" int boss_gp_fit(int device, int kernel, int d, int N, const double* X, const double* y,
                           const double* mean_X, const double* lengthscale, double amplitude, double noise_std,
                           const unsigned char* discrete, boss_gp_t** out, double* logpdf_out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    int rc = validate_hyper(d, lengthscale, amplitude, noise_std);
    if (rc) return rc;
    boss_gp_t* g = nullptr;
    rc = boss_gp_create(device, kernel, d, N, X, y, discrete, &g);
    if (rc) return rc;
    rc = boss_gp_update(g, lengthscale, amplitude, noise_std, mean_X, BOSS_FIT_DEFAULT, logpdf_out);
    if (rc) {
        std::string keep = g_last_error;
        boss_gp_free(g);
        g_last_error = keep;
        return rc;
    }
    *out = g;
    return BOSS_OK;
}

extern "C" void boss_gp_free(boss_gp_t* g) {
    if (!g) return;
    if (g->ctx) {
        (void)hipSetDevice(g->ctx->device);
        (void)hipStreamSynchronize(g->ctx->stream);
        if (g->dinv_pending) (void)hipEventSynchronize(g->dinv_ev);
    }
    gp_release(g);
}

extern "C" int boss_gp_n(const boss_gp_t* g, int* n_out) {
    if (!g || !n_out) return fail(BOSS_E_INVALID, "NULL argument");
    *n_out = g->N;
    return BOSS_OK;
}

extern "C" int boss_gp_get_factor(const boss_gp_t* g, double* L_out, double* z_out) {
    if (!g) return fail(BOSS_E_INVALID, "gp is NULL");
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    HIPCHK(hipSetDevice(g->ctx->device));
    std::lock_guard<std::mutex> lk(g->ctx->mtx);
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    const int N = g->N;
    if (L_out) {
        HIPCHK(hipMemcpy2D(L_out, sizeof(double) * N, g->A, sizeof(double) * g->ld, sizeof(double) * N, N,
                           hipMemcpyDeviceToHost));
        for (int j = 0; j < N; ++j)
            for (int i = 0; i < j; ++i) L_out[(size_t)j * N + i] = 0.0;
    }
    if (z_out) {
        HIPCHK(hipMemcpy2D(z_out, sizeof(double), g->A + g->Np, sizeof(double) * g->ld, sizeof(double), N,
                           hipMemcpyDeviceToHost));
    }
    return BOSS_OK;
}
