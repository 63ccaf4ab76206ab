// host_acqprog.inc — acquisition programs (boss_acqp_t) and the acquisition entry points built on them (included by bosship.hip).

struct boss_acqp {
    FitProg g;                                               // over 2P + Q inputs: μ[P] | σ²[P] | q[Q]
    int P, Q;
};

// ------------------------------------------------------------------------------------------
// the handle: validation only, no device
// ------------------------------------------------------------------------------------------
extern "C" int boss_acqp_create(int P, int Q, int n_const, const double* consts, int n_instr, const int* code, int out_id, boss_acqp_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (P < 1 || P > ACQP_MAXP) return fail(BOSS_E_INVALID, "an acquisition program takes the moments of 1 to 8 outputs");
    if (Q < 0 || Q > ACQP_MAXQ) return fail(BOSS_E_INVALID, "an acquisition program takes 0 to 16 runtime scalars");
    FitProg g;
    int rc = fit_build(2 * P + Q, n_const, consts, n_instr, code, out_id, "", "acquisition", ACQ_NOPS, &g);
    if (rc) return rc;
    boss_acqp* a = new boss_acqp();
    a->g = g;
    a->P = P;
    a->Q = Q;
    *out = a;
    return BOSS_OK;
}

extern "C" void boss_acqp_free(boss_acqp_t* acqp) { delete acqp; }

extern "C" int boss_acqp_eval_host(const boss_acqp_t* acqp, int n, const double* mu, const double* var, const double* q, double* a_out,
                                   double* da_dmu, double* da_dvar) {
    if (!acqp || n < 0 || (n > 0 && (!mu || !var || !a_out)) || (acqp->Q > 0 && !q)) return fail(BOSS_E_INVALID, "NULL argument");
    const FitProg& g = acqp->g;
    const int P = acqp->P, Q = acqp->Q;
    double y[2 * ACQP_MAXP + ACQP_MAXQ], ay[2 * ACQP_MAXP + ACQP_MAXQ], v[FIT_MAXI], av[FIT_MAXI];
    for (int k = 0; k < Q; ++k) y[2 * P + k] = q[k];
    for (int j = 0; j < n; ++j) {
        for (int p = 0; p < P; ++p) {
            y[p] = mu[(size_t)j * P + p];
            y[P + p] = var[(size_t)j * P + p];
        }
        a_out[j] = fit_eval<true>(g, y, v, 1);
        if (da_dmu || da_dvar) {
            fit_grad_sweep<false, true>(g, y, v, ay, av, 1);
            for (int p = 0; p < P; ++p) {
                if (da_dmu) da_dmu[(size_t)j * P + p] = ay[p];
                if (da_dvar) da_dvar[(size_t)j * P + p] = ay[P + p];
            }
        }
    }
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// launches (declared in bosship.hip for host_predict.inc / host_acq.inc)
// ------------------------------------------------------------------------------------------
// What every entry point checks before any device work, and the epilogue description it hands on.
static int acqp_check(const boss_acqp_t* acqp, int P, const double* q, double outside, AcqpEpi* pg) {
    if (!acqp) return fail(BOSS_E_INVALID, "NULL acquisition program");
    if (acqp->P != P) return fail(BOSS_E_INVALID, "the acquisition program takes the moments of " + std::to_string(acqp->P) + " outputs, the call has P = " + std::to_string(P));
    if (acqp->Q > 0 && !q) return fail(BOSS_E_INVALID, "the acquisition program takes " + std::to_string(acqp->Q) + " runtime scalars, q is NULL");
    pg->g = &acqp->g;
    pg->ap.P = acqp->P;
    pg->ap.Q = acqp->Q;
    for (int k = 0; k < ACQP_MAXQ; ++k) pg->ap.q[k] = k < acqp->Q ? q[k] : 0.0;
    pg->outside = outside;
    return BOSS_OK;
}

// workgroup size (whole waves, one candidate per thread) and dynamic LDS for a program: as many of the 4 waves as fit 64 KiB
static int acqp_block(const FitProg& g, bool grad, size_t* lds) {
    const size_t per_wave = sizeof(double) * 64 * (size_t)acqp_slots(g.P, g.nI, grad);
    const int waves = (int)std::max<size_t>(1, std::min<size_t>(ACQP_MAX_WAVES, (64 * 1024) / per_wave));
    *lds = per_wave * waves;
    return waves;
}

static void acqp_accumulate_launch(hipStream_t s, const double* mu, const double* var, size_t sstride, int ldm, int M, int s0, int s1,
                                   const AcqpEpi& pg, double* acq_sum, int add) {
    size_t lds;
    const int nt = 64 * acqp_block(*pg.g, false, &lds);
    hipLaunchKernelGGL(acqp_accumulate_kernel, dim3((M + nt - 1) / nt), dim3(nt), lds, s, mu, var, sstride, ldm, M, s0, s1, pg.ap, *pg.g, acq_sum, add);
}

static void acqp_grad_launch(hipStream_t s, const double* mu, const double* var, const double* dmu, const double* dvar, int M, int d, int S,
                             const AcqpEpi& pg, const unsigned char* mask, double* acq, double* dacq) {
    size_t lds;
    const int nt = 64 * acqp_block(*pg.g, true, &lds);
    hipLaunchKernelGGL(acqp_grad_set_kernel, dim3((M + nt - 1) / nt), dim3(nt), lds, s, mu, var, dmu, dvar, M, d, S, 1.0 / S, pg.ap, *pg.g, mask,
                       pg.outside, acq, dacq);
}

// ------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------
extern "C" int boss_acq_prog(int P, int S, boss_gp_t* const* gps, const boss_cand_t* cand, const double* mean_Xs, const boss_acqp_t* acqp,
                             const double* q, const unsigned char* valid_mask, double outside, double* acq_out, long* argmax_out,
                             double* max_out) {
    if (P < 1 || S < 1) return fail(BOSS_E_INVALID, "bad arguments");
    AcqpEpi pg;
    int rc = acqp_check(acqp, P, q, outside, &pg);
    if (rc) return rc;
    return acq_ei_impl(P, S, gps, cand, mean_Xs, nullptr, nullptr, 1, 0.0, valid_mask, acq_out, argmax_out, max_out, nullptr, 0, false, nullptr, &pg);
}

extern "C" int boss_acq_prog_grad(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs, const double* mean_grad,
                                  const boss_acqp_t* acqp, const double* q, const unsigned char* valid_mask, double outside, double* acq_out,
                                  double* dacq_out) {
    if (P < 1 || S < 1) return fail(BOSS_E_INVALID, "bad arguments");
    AcqpEpi pg;
    int rc = acqp_check(acqp, P, q, outside, &pg);
    if (rc) return rc;
    return acq_ei_grad_set_impl(P, S, gps, M, Xs, mean_Xs, mean_grad, nullptr, nullptr, 1, 0.0, valid_mask, acq_out, dacq_out, nullptr, &pg);
}

// From moments on the host: mu / var S×P×M as boss_acq_ei_moments takes them.
extern "C" int boss_acq_prog_moments(int device, int P, int S, int M, const double* mu, const double* var, const boss_acqp_t* acqp,
                                     const double* q, const unsigned char* valid_mask, double outside, double* acq_out, long* argmax_out,
                                     double* max_out) {
    if (P < 1 || S < 1 || M < 1 || !mu || !var) return fail(BOSS_E_INVALID, "bad arguments");
    AcqpEpi pg;
    int rc = acqp_check(acqp, P, q, outside, &pg);
    if (rc) return rc;
    if ((long long)P * S * M > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M above 2^30 is not supported");
    Ctx* c;
    rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const size_t pm = (size_t)P * M;
    const size_t nd = 2 * pm * S + M;                        // mu | var | acq | mask
    rc = ws_reserve(c->acq, sizeof(double) * nd + M);
    if (rc) return rc;
    double* dmu = (double*)c->acq.p;
    double* dvar = dmu + pm * S;
    double* dacq = dvar + pm * S;
    unsigned char* dmask = (unsigned char*)(dmu + nd);
    double* hres = (double*)c->pinned;
    EiPar par;
    const double no_coefs[EI_MAXP] = {};
    rc = ei_params(c, s, P, no_coefs, nullptr, 1, 0.0, &par, nullptr, nullptr);   // (P <= EI_MAXP: by value; the epilogue runs it in mode 0)
    if (rc) return rc;
    (void)hipMemcpyAsync(dmu, mu, sizeof(double) * pm * S, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(dvar, var, sizeof(double) * pm * S, hipMemcpyHostToDevice, s);
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    ei_value_epilogue_launch(s, dmu, dvar, M, S, par, nullptr, nullptr, valid_mask ? dmask : nullptr, nullptr, nullptr, dacq, hres, 0ull, nullptr, 0, &pg);
    if (acq_out) (void)hipMemcpyAsync(acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    hipError_t e2 = hipGetLastError();
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e2));
    if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
    if (max_out) *max_out = hres[0];
    return BOSS_OK;
}

// From moments and moment gradients on the host: mu / var [s][p][M], dmu / dvar [s][p][d×M] (boss_acq_ei_mc_grad_moments' layouts).
extern "C" int boss_acq_prog_grad_moments(int device, int P, int S, int M, int d, const double* mu, const double* var, const double* dmu,
                                          const double* dvar, const boss_acqp_t* acqp, const double* q, const unsigned char* valid_mask,
                                          double outside, double* acq_out, double* dacq_out) {
    if (P < 1 || S < 1 || M < 1 || d < 1 || !mu || !var || !dmu || !dvar || !acq_out || !dacq_out) return fail(BOSS_E_INVALID, "bad arguments");
    AcqpEpi pg;
    int rc = acqp_check(acqp, P, q, outside, &pg);
    if (rc) return rc;
    if ((long long)P * S * M * d > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M·d above 2^30 is not supported");
    Ctx* c;
    rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const size_t dm = (size_t)d * M, nm = (size_t)P * S * M, ndm = nm * d;
    const size_t nd = 2 * nm + 2 * ndm + M + dm;             // mu | var | dmu | dvar | acq | dacq | mask
    rc = ws_reserve(c->pred, sizeof(double) * nd + M);
    if (rc) return rc;
    double* d_mu = (double*)c->pred.p;
    double* d_var = d_mu + nm;
    double* d_gm = d_var + nm;
    double* d_gv = d_gm + ndm;
    double* dacq = d_gv + ndm;
    double* ddacq = dacq + M;
    unsigned char* dmask = (unsigned char*)(d_mu + nd);
    (void)hipMemcpyAsync(d_mu, mu, sizeof(double) * nm, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_var, var, sizeof(double) * nm, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_gm, dmu, sizeof(double) * ndm, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_gv, dvar, sizeof(double) * ndm, hipMemcpyHostToDevice, s);
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    acqp_grad_launch(s, d_mu, d_var, d_gm, d_gv, M, d, S, pg, valid_mask ? dmask : nullptr, dacq, ddacq);
    return finish(c, {{acq_out, dacq, sizeof(double) * M}, {dacq_out, ddacq, sizeof(double) * dm}});
}
