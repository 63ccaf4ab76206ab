// host_warp.inc — warps (boss_warp_t): the handle, the host twins of the two stages and their device calls (included by bosship.hip).

struct boss_warp {
    int d_user = 0, d_model = 0, P = 0, nI_in = 0, nI_out = 0;   // d_user = d_model = 0 without an input program
    std::vector<FitProg> gin;                                // d_model programs over d_user inputs, or empty = the identity
    std::vector<FitProg> gout;                               // 2P programs over (μ_0.., σ_0..), or empty = the identity
};

// ------------------------------------------------------------------------------------------
// the handle: validation and copies only, no device
// ------------------------------------------------------------------------------------------
extern "C" int boss_warp_create(const boss_mean_t* in_prog, int P, const boss_mean_t* out_prog, boss_warp_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!in_prog && !out_prog) return fail(BOSS_E_INVALID, "a warp needs an input program, an output program or both");
    const int maxP = out_prog ? WARP_MAXP : EI_MAXP;
    if (P < 1 || P > maxP)
        return fail(BOSS_E_INVALID, out_prog ? "a warp with an output program has 1 to 8 outputs (2P program outputs, at most 16)"
                                             : "a warp has 1 to 16 outputs");
    if (in_prog) {
        if (in_prog->T != 0) return fail(BOSS_E_INVALID, "input program: a warp program takes no parameters (T must be 0)");
        if (in_prog->d > WARP_MAXD)
            return fail(BOSS_E_INVALID, "input program: " + std::to_string(in_prog->d) + " inputs, a warp takes x_dim <= 16");
    }
    if (out_prog) {
        if (out_prog->T != 0) return fail(BOSS_E_INVALID, "output program: a warp program takes no parameters (T must be 0)");
        if (out_prog->d != 2 * P)
            return fail(BOSS_E_INVALID, "output program: " + std::to_string(out_prog->d) + " inputs, 2P = " + std::to_string(2 * P) +
                                            " expected (the means, then the standard deviations)");
        if (out_prog->P != 2 * P)
            return fail(BOSS_E_INVALID, "output program: " + std::to_string(out_prog->P) + " outputs, 2P = " + std::to_string(2 * P) +
                                            " expected (the means, then the standard deviations)");
    }
    boss_warp* w = new boss_warp();
    w->P = P;
    if (in_prog) {
        w->d_user = in_prog->d;
        w->d_model = in_prog->P;
        w->nI_in = in_prog->nI_max;
        w->gin = in_prog->g;
    }
    if (out_prog) {
        w->nI_out = out_prog->nI_max;
        w->gout = out_prog->g;
    }
    *out = w;
    return BOSS_OK;
}

extern "C" void boss_warp_free(boss_warp_t* w) { delete w; }

// ------------------------------------------------------------------------------------------
// argument checks shared by the host twins and the device calls
// ------------------------------------------------------------------------------------------
static int warp_apply_check(const boss_warp_t* w, int M, const double* Xs, const double* X_out) {
    if (!w) return fail(BOSS_E_INVALID, "NULL warp");
    if (w->gin.empty()) return fail(BOSS_E_INVALID, "the warp has no input program");
    if (M < 1 || !Xs || !X_out) return fail(BOSS_E_INVALID, "M must be >= 1, Xs and X_out not NULL");
    if ((long long)M * w->d_model * w->d_user > (1LL << 30)) return fail(BOSS_E_INVALID, "M·d_model·d_user above 2^30 is not supported");
    return BOSS_OK;
}

// *d_model_out: the dimension the model-space gradients have; *grad_out: whether gradients travel
static int warp_moments_check(const boss_warp_t* w, int S, int M, int d_user, const double* mu_, const double* var_, const double* dmu_,
                              const double* dvar_, const double* jac, const double* mu, const double* var, const double* dmu,
                              const double* dvar, int* d_model_out, bool* grad_out) {
    if (!w) return fail(BOSS_E_INVALID, "NULL warp");
    if (S < 1 || M < 1) return fail(BOSS_E_INVALID, "S and M must be >= 1");
    if (d_user < 1 || d_user > WARP_MAXD) return fail(BOSS_E_INVALID, "d_user must be 1 to 16");
    if (!mu_ || !var_ || !mu || !var) return fail(BOSS_E_INVALID, "NULL moments");
    const int ng = (dmu_ ? 1 : 0) + (dvar_ ? 1 : 0) + (dmu ? 1 : 0) + (dvar ? 1 : 0);
    if (ng != 0 && ng != 4) return fail(BOSS_E_INVALID, "dmu_, dvar_, dmu and dvar must be all NULL or all given");
    if (jac && ng == 0) return fail(BOSS_E_INVALID, "jac given without the gradient arrays");
    int d_model = d_user;
    if (!w->gin.empty()) {
        if (d_user != w->d_user)
            return fail(BOSS_E_INVALID, "d_user = " + std::to_string(d_user) + ", the warp's input program takes " + std::to_string(w->d_user));
        if (ng && !jac) return fail(BOSS_E_INVALID, "jac is NULL: gradients through a warp with an input program need its Jacobians");
        d_model = w->d_model;
    } else if (jac)
        return fail(BOSS_E_INVALID, "jac given, the warp has no input program");
    if ((long long)S * w->P * M * std::max(d_model, d_user) > (1LL << 30))
        return fail(BOSS_E_INVALID, "S·P·M·max(d_model, d_user) above 2^30 is not supported");
    *d_model_out = d_model;
    *grad_out = ng != 0;
    return BOSS_OK;
}

// the predict convention (bad_index given): the first variance below the clip, in memory order [s][p][j], fails the call
static int warp_neg_var_scan(int S, int P, int M, const double* var_, long* bad_index) {
    const size_t n = (size_t)S * P * M;
    for (size_t i = 0; i < n; ++i)
        if (var_[i] < -MAX_NEG_VAR) return neg_var_error(bad_index, (unsigned long long)(i % M), var_[i]);
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// host twins (tests, no device): the kernels' loops over the same __host__ __device__ functions on unit-stride columns
// ------------------------------------------------------------------------------------------
extern "C" int boss_warp_apply_host(const boss_warp_t* w, int M, const double* Xs, double* X_out, double* jac_out) {
    int rc = warp_apply_check(w, M, Xs, X_out);
    if (rc) return rc;
    const int du = w->d_user, dm = w->d_model;
    double col[warp_x_slots(WARP_MAXD, FIT_MAXI, true)];
    for (int j = 0; j < M; ++j) {
        if (jac_out)
            warp_x_point<true>(w->gin.data(), du, dm, w->nI_in, Xs + (size_t)j * du, col, 1, X_out + (size_t)j * dm, 1, jac_out + (size_t)j * dm * du);
        else
            warp_x_point<false>(w->gin.data(), du, dm, w->nI_in, Xs + (size_t)j * du, col, 1, X_out + (size_t)j * dm, 1, nullptr);
    }
    return BOSS_OK;
}

extern "C" int boss_warp_moments_host(const boss_warp_t* w, int S, int M, int d_user, const double* mu_, const double* var_,
                                      const double* dmu_, const double* dvar_, const double* jac, double* mu, double* var, double* dmu,
                                      double* dvar, long* bad_index) {
    int dm;
    bool grad;
    int rc = warp_moments_check(w, S, M, d_user, mu_, var_, dmu_, dvar_, jac, mu, var, dmu, dvar, &dm, &grad);
    if (rc) return rc;
    const int P = w->P, du = d_user;
    if (bad_index) {
        rc = warp_neg_var_scan(S, P, M, var_, bad_index);
        if (rc) return rc;
    }
    const FitProg* gout = w->gout.empty() ? nullptr : w->gout.data();
    const size_t pm = (size_t)P * M, pdm = pm * dm, pdu = pm * du;
    double col[warp_m_slots(EI_MAXP, FIT_MAXI, WARP_MAXD, true)];
    for (int s = 0; s < S; ++s)
        for (int r = 0; r < 2 * P; ++r)
            for (int j = 0; j < M; ++j) {
                const double* Jj = jac ? jac + (size_t)j * dm * du : nullptr;
                if (grad)
                    warp_moments_point<true>(gout, P, r, w->nI_out, M, dm, du, mu_ + s * pm, var_ + s * pm, dmu_ + s * pdm, dvar_ + s * pdm, Jj,
                                             j, col, 1, mu + s * pm, var + s * pm, dmu + s * pdu, dvar + s * pdu);
                else
                    warp_moments_point<false>(gout, P, r, w->nI_out, M, dm, du, mu_ + s * pm, var_ + s * pm, nullptr, nullptr, nullptr, j, col,
                                              1, mu + s * pm, var + s * pm, nullptr, nullptr);
            }
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// launches.  Workgroup shape as for a mean program: whole waves, one candidate per thread, as many of the 4 waves as fit 64 KiB
// and no more than the candidates need; one wave of the longest program takes what it takes (80 KiB and 88 KiB at the limits).
// ------------------------------------------------------------------------------------------
static int warp_waves(int slots, int n, size_t* lds) {
    const size_t per_wave = sizeof(double) * 64 * (size_t)std::max(1, slots);
    int waves = (int)std::max<size_t>(1, std::min<size_t>(WARP_MAX_WAVES, (64 * 1024) / per_wave));
    waves = std::max(1, std::min(waves, (n + 63) / 64));
    *lds = per_wave * waves;
    return waves;
}

// (tests) the workgroup shape of a stage for n candidates: stage 0 = warp_x_kernel, 1 = warp_moments_kernel (d_model: the gradient
// slots of its column; ignored otherwise); waves per workgroup, dynamic LDS bytes in *lds_out
extern "C" int boss_debug_warp_block(const boss_warp_t* w, int stage, int grad, int n, int d_model, int* lds_out) {
    if (!w || n < 1 || (stage == 0 && w->gin.empty())) return 0;
    size_t lds;
    const int slots = stage == 0 ? warp_x_slots(w->d_user, w->nI_in, grad != 0) : warp_m_slots(w->P, w->nI_out, d_model, grad != 0);
    const int waves = warp_waves(slots, n, &lds);
    if (lds_out) *lds_out = (int)lds;
    return waves;
}

// dXs d_user×M on the device -> dX_ (coordinate r of candidate j at r*xs_r + j*xs_j) and dJ (NULL: no sweep).  dprogs: the d_model
// programs on the device.  Enqueue only.
static void warp_x_enqueue(hipStream_t s, const boss_warp* w, const FitProg* dprogs, const double* dXs, int M, double* dX_, size_t xs_r,
                           size_t xs_j, double* dJ) {
    size_t lds;
    const int waves = warp_waves(warp_x_slots(w->d_user, w->nI_in, dJ != nullptr), M, &lds);
    const dim3 grid((M + 64 * waves - 1) / (64 * waves)), block(64 * waves);
    // (only a long program's single wave goes beyond the 64 KiB a launch may ask for without this; set where it is needed, not in ctx_init)
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)warp_x_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, WARP_X_MAX_LDS);
    if (dJ)
        hipLaunchKernelGGL(warp_x_kernel<true>, grid, block, lds, s, dprogs, dXs, M, w->d_user, w->d_model, w->nI_in, dX_, xs_r, xs_j, dJ);
    else
        hipLaunchKernelGGL(warp_x_kernel<false>, grid, block, lds, s, dprogs, dXs, M, w->d_user, w->d_model, w->nI_in, dX_, xs_r, xs_j, (double*)nullptr);
}

// device-resident moments of S samples through the output programs (dprogs NULL: the identity) and Jᵀ.  Enqueue only.
static void warp_moments_enqueue(hipStream_t s, const boss_warp* w, const FitProg* dprogs, int S, int M, int d_model, int d_user,
                                 const double* mu_, const double* var_, const double* dmu_, const double* dvar_, const double* dJ, double* mu,
                                 double* var, double* dmu, double* dvar) {
    const bool grad = dmu_ != nullptr;
    size_t lds;
    const int waves = warp_waves(warp_m_slots(w->P, w->nI_out, d_model, grad), M, &lds);
    const dim3 grid((M + 64 * waves - 1) / (64 * waves), 2 * w->P, std::min(S, 65535)), block(64 * waves);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)warp_moments_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, WARP_M_MAX_LDS);
    if (grad)
        hipLaunchKernelGGL(warp_moments_kernel<true>, grid, block, lds, s, dprogs, w->P, w->nI_out, S, M, d_model, d_user, mu_, var_, dmu_,
                           dvar_, dJ, mu, var, dmu, dvar);
    else
        hipLaunchKernelGGL(warp_moments_kernel<false>, grid, block, lds, s, dprogs, w->P, w->nI_out, S, M, d_model, d_user, mu_, var_,
                           (const double*)nullptr, (const double*)nullptr, (const double*)nullptr, mu, var, (double*)nullptr, (double*)nullptr);
}

static int warp_finish(hipStream_t s) {
    hipError_t e = hipStreamSynchronize(s);
    const hipError_t e2 = hipGetLastError();                 // (read either way: it also clears the error)
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// the two stages on host arrays (tests and the Python layer's staged paths)
// ------------------------------------------------------------------------------------------
extern "C" int boss_warp_apply(int device, const boss_warp_t* w, int M, const double* Xs, double* X_out, double* jac_out) {
    int rc = warp_apply_check(w, M, Xs, X_out);
    if (rc) return rc;
    Ctx* c;
    rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const int du = w->d_user, dm = w->d_model;
    const size_t prog_bytes = sizeof(FitProg) * (size_t)dm;  // (a multiple of 8)
    const size_t n_x = (size_t)du * M, n_o = (size_t)dm * M, n_j = jac_out ? n_o * du : 0;
    // programs | Xs | X_ | J
    rc = ws_reserve(c->warpws, prog_bytes + sizeof(double) * (n_x + n_o + n_j));
    if (rc) return rc;
    FitProg* dprogs = (FitProg*)c->warpws.p;
    double* dXs = (double*)((char*)c->warpws.p + prog_bytes);
    double* dX_ = dXs + n_x;
    double* dJ = dX_ + n_o;
    (void)hipMemcpyAsync(dprogs, w->gin.data(), prog_bytes, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(dXs, Xs, sizeof(double) * n_x, hipMemcpyHostToDevice, s);
    warp_x_enqueue(s, w, dprogs, dXs, M, dX_, 1, (size_t)dm, jac_out ? dJ : nullptr);
    (void)hipMemcpyAsync(X_out, dX_, sizeof(double) * n_o, hipMemcpyDeviceToHost, s);
    if (jac_out) (void)hipMemcpyAsync(jac_out, dJ, sizeof(double) * n_j, hipMemcpyDeviceToHost, s);
    return warp_finish(s);
}

extern "C" int boss_warp_moments(int device, const boss_warp_t* w, int S, int M, int d_user, const double* mu_, const double* var_,
                                 const double* dmu_, const double* dvar_, const double* jac, double* mu, double* var, double* dmu,
                                 double* dvar, long* bad_index) {
    int dm;
    bool grad;
    int rc = warp_moments_check(w, S, M, d_user, mu_, var_, dmu_, dvar_, jac, mu, var, dmu, dvar, &dm, &grad);
    if (rc) return rc;
    const int P = w->P, du = d_user;
    if (bad_index) {
        rc = warp_neg_var_scan(S, P, M, var_, bad_index);
        if (rc) return rc;
    }
    Ctx* c;
    rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const size_t prog_bytes = sizeof(FitProg) * w->gout.size();
    const size_t n_m = (size_t)S * P * M, n_gi = grad ? n_m * dm : 0, n_go = grad ? n_m * du : 0, n_j = jac ? (size_t)M * dm * du : 0;
    // programs | mu_ | var_ | dmu_ | dvar_ | J | mu | var | dmu | dvar
    rc = ws_reserve(c->warpws, prog_bytes + sizeof(double) * (4 * n_m + 2 * n_gi + 2 * n_go + n_j));
    if (rc) return rc;
    FitProg* dprogs = (FitProg*)c->warpws.p;
    double* i_mu = (double*)((char*)c->warpws.p + prog_bytes);
    double* i_var = i_mu + n_m;
    double* i_dmu = i_var + n_m;
    double* i_dvar = i_dmu + n_gi;
    double* dJ = i_dvar + n_gi;
    double* o_mu = dJ + n_j;
    double* o_var = o_mu + n_m;
    double* o_dmu = o_var + n_m;
    double* o_dvar = o_dmu + n_go;
    if (prog_bytes) (void)hipMemcpyAsync(dprogs, w->gout.data(), prog_bytes, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(i_mu, mu_, sizeof(double) * n_m, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(i_var, var_, sizeof(double) * n_m, hipMemcpyHostToDevice, s);
    if (grad) {
        (void)hipMemcpyAsync(i_dmu, dmu_, sizeof(double) * n_gi, hipMemcpyHostToDevice, s);
        (void)hipMemcpyAsync(i_dvar, dvar_, sizeof(double) * n_gi, hipMemcpyHostToDevice, s);
    }
    if (jac) (void)hipMemcpyAsync(dJ, jac, sizeof(double) * n_j, hipMemcpyHostToDevice, s);
    warp_moments_enqueue(s, w, prog_bytes ? dprogs : nullptr, S, M, dm, du, i_mu, i_var, grad ? i_dmu : nullptr, grad ? i_dvar : nullptr,
                         jac ? dJ : nullptr, o_mu, o_var, grad ? o_dmu : nullptr, grad ? o_dvar : nullptr);
    (void)hipMemcpyAsync(mu, o_mu, sizeof(double) * n_m, hipMemcpyDeviceToHost, s);
    (void)hipMemcpyAsync(var, o_var, sizeof(double) * n_m, hipMemcpyDeviceToHost, s);
    if (grad) {
        (void)hipMemcpyAsync(dmu, o_dmu, sizeof(double) * n_go, hipMemcpyDeviceToHost, s);
        (void)hipMemcpyAsync(dvar, o_dvar, sizeof(double) * n_go, hipMemcpyDeviceToHost, s);
    }
    return warp_finish(s);
}

// ------------------------------------------------------------------------------------------
// one-call paths: boss_warp_predict, boss_warp_predict_grad, boss_acq_ei_warp, boss_acq_ei_grad_warp — one enqueue path, as the
// nonstationary set calls have (ngp_grad_set_call).  Xs goes up once, warp_x_kernel writes the rows of a temporary candidate set,
// the members' prediction of the plain calls runs on it unchanged (members_enqueue), warp_moments_kernel takes the device-resident
// moments of every sample to user space, and the epilogues of the plain calls (ei_value_epilogue_launch, ei_grad_epilogue_launch)
// run on the result: y_max, best and the arg-max are in user space.  One copy back.  tests/test_gpu_warp.py holds these paths to
// the plain calls' bits.
// ------------------------------------------------------------------------------------------
struct WarpAcq {
    const double* fit_coefs;
    const double* y_max;
    int has_best;
    double best;
    const unsigned char* valid_mask;
    double* acq_out;
    long* argmax_out;                                        // (value call)
    double* max_out;
    double* dacq_out;                                        // (gradient call)
};

static int warp_call(const boss_warp_t* w, int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                     const double* mean_grad, bool grad, const WarpAcq* acq, double* mu, double* var, double* dmu, double* dvar,
                     long* bad_index) {
    if (!w) return fail(BOSS_E_INVALID, "NULL warp");
    if (P < 1 || S < 1 || !gps || M < 1 || !Xs) return fail(BOSS_E_INVALID, "bad arguments");
    if (P != w->P) return fail(BOSS_E_INVALID, "P = " + std::to_string(P) + ", the warp was created for " + std::to_string(w->P) + " outputs");
    if (acq ? (!acq->fit_coefs || (grad && (!acq->acq_out || !acq->dacq_out))) : (!mu || !var || (grad && (!dmu || !dvar))))
        return fail(BOSS_E_INVALID, "NULL argument");
    if (bad_index) *bad_index = -1;
    const int n = P * S;
    const bool has_in = !w->gin.empty(), has_out = !w->gout.empty();
    for (int i = 0; i < n; ++i) {
        if (!gps[i]) return fail(BOSS_E_INVALID, "NULL posterior handle");
        NOT_FOR_GIBBS(gps[i], mean_Xs, mean_grad);
        if (gps[i]->ctx != gps[0]->ctx || gps[i]->d != gps[0]->d)
            return fail(BOSS_E_INVALID, "all handles must live on one device and share x_dim");
    }
    for (int i = 0; i < n; ++i)
        if (!gps[i]->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
    const int dm = gps[0]->d, du = has_in ? w->d_user : dm;
    if (has_in && dm != w->d_model)
        return fail(BOSS_E_INVALID, "the handles have x_dim = " + std::to_string(dm) + ", the warp's input program has " +
                                        std::to_string(w->d_model) + " outputs");
    if (dm > WARP_MAXD) return fail(BOSS_E_INVALID, "x_dim above 16 is not supported under a warp");
    if ((long long)n * M * std::max(dm, du) > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M·max(d_model, d_user) above 2^30 is not supported");
    Ctx* c = gps[0]->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    // programs and what the input warp reads and leaves: in programs | out programs | Xs | J
    const size_t in_bytes = sizeof(FitProg) * w->gin.size(), out_bytes = sizeof(FitProg) * w->gout.size();
    const size_t n_x = has_in ? (size_t)du * M : 0, n_j = has_in && grad ? (size_t)M * dm * du : 0;
    int rc = ws_reserve(c->warpws, in_bytes + out_bytes + sizeof(double) * (n_x + n_j));
    if (rc) return rc;
    FitProg* din = (FitProg*)c->warpws.p;
    FitProg* dout = (FitProg*)((char*)c->warpws.p + in_bytes);
    double* dXs = (double*)((char*)c->warpws.p + in_bytes + out_bytes);
    double* dJ = n_j ? dXs + n_x : nullptr;
    if (out_bytes) (void)hipMemcpyAsync(dout, w->gout.data(), out_bytes, hipMemcpyHostToDevice, s);
    boss_cand cd;
    if (has_in) {
        cd.ctx = c;
        cd.d = dm;
        cd.M = M;
        cd.Mp = round_up(M, 64);
        rc = ws_reserve(c->craw, sizeof(double) * (size_t)dm * cd.Mp);
        if (rc) return drain(c, rc);
        cd.Craw = (double*)c->craw.p;
        (void)hipMemcpyAsync(din, w->gin.data(), in_bytes, hipMemcpyHostToDevice, s);
        (void)hipMemcpyAsync(dXs, Xs, sizeof(double) * n_x, hipMemcpyHostToDevice, s);
        (void)hipMemsetAsync(cd.Craw, 0, sizeof(double) * (size_t)dm * cd.Mp, s);   // (the padding columns, as pack_points leaves them)
        warp_x_enqueue(s, w, din, dXs, M, cd.Craw, (size_t)cd.Mp, 1, dJ);
    } else {
        rc = temp_cand(c, dm, M, Xs, &cd);
        if (rc) return drain(c, rc);
    }
    const size_t nm = (size_t)n * M, gi = grad ? nm * dm : 0, go = grad ? nm * du : 0, duM = (size_t)du * M;
    // the moments kernel runs unless it would copy: no output program and no gradient to take through J'
    const bool fold = has_out || (grad && has_in);
    // device scratch: user space first (what travels back lies together): mu | var | dmu | dvar | bad | acq | dacq |
    // model space: mu_ | var_ | dmu_ | dvar_ | mean | mean_grad | coefs | ymax | mask
    const size_t nd = 2 * nm + 2 * go + 1 + M + duM + (fold ? 2 * nm + 2 * gi : 0) + nm + gi + 2 * (size_t)P;
    rc = ws_reserve(c->pred, sizeof(double) * nd + M);
    if (rc) return drain(c, rc);
    double* o_mu = (double*)c->pred.p;
    double* o_var = o_mu + nm;
    double* o_gm = o_var + nm;
    double* o_gv = o_gm + go;
    unsigned long long* dbad = (unsigned long long*)(o_gv + go);
    double* dacq = o_gv + go + 1;
    double* ddacq = dacq + M;
    double* i_mu = fold ? ddacq + duM : o_mu;
    double* i_var = fold ? i_mu + nm : o_var;
    double* i_gm = fold ? i_var + nm : o_gm;
    double* i_gv = fold ? i_gm + gi : o_gv;
    double* dmean = fold ? i_gv + gi : ddacq + duM;
    double* dmg = dmean + nm;
    double* dcoef = dmg + gi;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(o_mu + nd);
    EiPar par;
    par.mode = 1;                                            // (the prediction calls always predict)
    if (acq) {
        rc = ei_params(c, s, P, acq->fit_coefs, acq->y_max, acq->has_best, acq->best, &par, dcoef, dymax);
        if (rc) return drain(c, rc);
        if (acq->valid_mask) (void)hipMemcpyAsync(dmask, acq->valid_mask, M, hipMemcpyHostToDevice, s);
    }
    if (mean_Xs) (void)hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * nm, hipMemcpyHostToDevice, s);
    if (mean_grad && grad) (void)hipMemcpyAsync(dmg, mean_grad, sizeof(double) * gi, hipMemcpyHostToDevice, s);
    if (par.mode != 0) {
        MemberSlices q;
        q.mean = mean_Xs ? dmean : nullptr;
        q.mean_grad = mean_grad && grad ? dmg : nullptr;
        q.mu = i_mu, q.var = i_var, q.gm = grad ? i_gm : nullptr, q.gv = grad ? i_gv : nullptr;
        rc = members_enqueue(n, gps, &cd, q, acq && S > 1);  // (S = 1 and the prediction calls: member by member, as the plain calls)
        if (rc) return drain(c, rc);
        if (!acq) {
            // the prediction calls' convention for a variance below the clip, on the model's own variances (member i = p + P·s at i·M)
            (void)hipMemsetAsync(dbad, 0xff, sizeof(unsigned long long), s);
            hipLaunchKernelGGL(clip_var_kernel, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, s, i_var, (int)nm, dbad);
        }
        if (fold)
            warp_moments_enqueue(s, w, has_out ? dout : nullptr, S, M, dm, du, i_mu, i_var, grad ? i_gm : nullptr, grad ? i_gv : nullptr,
                                 has_in && grad ? dJ : nullptr, o_mu, o_var, grad ? o_gm : nullptr, grad ? o_gv : nullptr);
    }
    if (!acq) {
        unsigned long long bad = 0;
        if (grad)
            rc = finish(c, {{mu, o_mu, sizeof(double) * nm}, {var, o_var, sizeof(double) * nm}, {dmu, o_gm, sizeof(double) * go},
                            {dvar, o_gv, sizeof(double) * go}, {&bad, dbad, sizeof bad}});
        else
            rc = finish(c, {{mu, o_mu, sizeof(double) * nm}, {var, o_var, sizeof(double) * nm}, {&bad, dbad, sizeof bad}});
        if (rc) return rc;
        if (bad == ~0ULL) return BOSS_OK;
        double v = 0.0;                                      // (the model's variance there: the user-space one may have any value)
        HIPCHK(hipMemcpy(&v, i_var + bad, sizeof v, hipMemcpyDeviceToHost));
        return neg_var_error(bad_index, bad % (unsigned long long)M, v);
    }
    const unsigned char* mk = acq->valid_mask ? dmask : nullptr;
    if (grad) {
        ei_grad_epilogue_launch(s, o_mu, o_var, o_gm, o_gv, M, du, S, S == 1, par, dcoef, dymax, mk, nullptr, nullptr, dacq, ddacq);
        return finish(c, {{acq->acq_out, dacq, sizeof(double) * M}, {acq->dacq_out, ddacq, sizeof(double) * duM}});
    }
    double* hres = (double*)c->pinned;
    ei_value_epilogue_launch(s, o_mu, o_var, M, S, par, dcoef, dymax, mk, nullptr, nullptr, dacq, hres, 0ull);
    if (acq->acq_out) (void)hipMemcpyAsync(acq->acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, s);
    rc = warp_finish(s);
    if (rc) return rc;
    if (acq->argmax_out) std::memcpy(acq->argmax_out, &hres[1], sizeof(long));
    if (acq->max_out) *acq->max_out = hres[0];
    return BOSS_OK;
}

extern "C" int boss_warp_predict(const boss_warp_t* w, int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                 double* mu, double* var, long* bad_index) {
    return warp_call(w, P, S, gps, M, Xs, mean_Xs, nullptr, false, nullptr, mu, var, nullptr, nullptr, bad_index);
}

extern "C" int boss_warp_predict_grad(const boss_warp_t* w, int P, int S, boss_gp_t* const* gps, int M, const double* Xs,
                                      const double* mean_Xs, const double* mean_grad, double* mu, double* var, double* dmu, double* dvar,
                                      long* bad_index) {
    return warp_call(w, P, S, gps, M, Xs, mean_Xs, mean_grad, true, nullptr, mu, var, dmu, dvar, bad_index);
}

extern "C" int boss_acq_ei_warp(const boss_warp_t* w, int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                const double* fit_coefs, const double* y_max, int has_best, double best, const unsigned char* valid_mask,
                                double* acq_out, long* argmax_out, double* max_out) {
    const WarpAcq a{fit_coefs, y_max, has_best, best, valid_mask, acq_out, argmax_out, max_out, nullptr};
    return warp_call(w, P, S, gps, M, Xs, mean_Xs, nullptr, false, &a, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int boss_acq_ei_grad_warp(const boss_warp_t* w, int P, int S, boss_gp_t* const* gps, int M, const double* Xs,
                                     const double* mean_Xs, const double* mean_grad, const double* fit_coefs, const double* y_max,
                                     int has_best, double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    const WarpAcq a{fit_coefs, y_max, has_best, best, valid_mask, acq_out, nullptr, nullptr, dacq_out};
    return warp_call(w, P, S, gps, M, Xs, mean_Xs, mean_grad, true, &a, nullptr, nullptr, nullptr, nullptr, nullptr);
}
