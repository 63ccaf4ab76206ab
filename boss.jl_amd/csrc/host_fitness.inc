// host_fitness.inc — fitness programs (boss_fit_t) and the Monte-Carlo EI entry points built on them (included by bosship.hip).

struct boss_fit {
    FitProg g;
};

// ------------------------------------------------------------------------------------------
// the handle: validation only, no device
// ------------------------------------------------------------------------------------------
// The checks of a program over n_in inputs, shared with boss_mean_create (host_mean.inc): `pre` is put in front of every message
// (a mean program names its output there), `what` names the kind of program.
// n_ops: how many opcodes the caller's kind of program knows (FIT_NOPS; ACQ_NOPS for acquisition programs, host_acqprog.inc).
static int fit_build(int n_in, int n_const, const double* consts, int n_instr, const int* code, int out_id, const std::string& pre,
                     const char* what, int n_ops, FitProg* out) {
    if (n_const < 0 || n_const > FIT_MAXC) return fail(BOSS_E_INVALID, pre + "a " + what + " program holds at most 32 constants");
    if (n_instr < 0 || n_instr > FIT_MAXI) return fail(BOSS_E_INVALID, pre + "a " + what + " program holds at most 64 instructions");
    if ((n_const > 0 && !consts) || (n_instr > 0 && !code)) return fail(BOSS_E_INVALID, pre + "NULL constants or code");
    FitProg g;
    std::memset(&g, 0, sizeof g);
    g.P = n_in;
    g.nC = n_const;
    g.nI = n_instr;
    for (int k = 0; k < n_const; ++k) {
        if (!std::isfinite(consts[k])) return fail(BOSS_E_INVALID, pre + "constant " + std::to_string(k) + " of the " + what + " program is not finite");
        g.c[k] = consts[k];
    }
    const int base = n_in + n_const;
    for (int i = 0; i < n_instr; ++i) {
        const int op = code[3 * i], a = code[3 * i + 1], b = code[3 * i + 2];
        const std::string at = pre + "instruction " + std::to_string(i) + ": ";
        if (op < 0 || op >= n_ops) return fail(BOSS_E_INVALID, at + "unknown opcode " + std::to_string(op));
        if (a < 0 || a >= base + i) return fail(BOSS_E_INVALID, at + "operand a must be an earlier value id");
        if (fit_is_unary(op)) {
            if (b != -1) return fail(BOSS_E_INVALID, at + "a unary operation takes b = -1");
        } else if (b < 0 || b >= base + i) {
            return fail(BOSS_E_INVALID, at + "operand b must be an earlier value id");
        }
        g.op[i] = (unsigned char)op;
        g.a[i] = (unsigned char)a;
        g.b[i] = (unsigned char)(b < 0 ? FIT_NOARG : b);
    }
    if (out_id < 0 || out_id >= base + n_instr) return fail(BOSS_E_INVALID, pre + "out_id is not a value id of the program");
    g.out = out_id;
    *out = g;
    return BOSS_OK;
}

extern "C" int boss_fit_create(int P, int n_const, const double* consts, int n_instr, const int* code, int out_id, boss_fit_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (P < 1 || P > EI_MAXP) return fail(BOSS_E_INVALID, "a fitness program takes 1 to 16 inputs");
    FitProg g;
    int rc = fit_build(P, n_const, consts, n_instr, code, out_id, "", "fitness", FIT_NOPS, &g);
    if (rc) return rc;
    boss_fit* f = new boss_fit();
    f->g = g;
    *out = f;
    return BOSS_OK;
}

extern "C" void boss_fit_free(boss_fit_t* fit) { delete fit; }

extern "C" int boss_fit_eval_host(const boss_fit_t* fit, int n, const double* Y, double* f_out, double* df_out) {
    if (!fit || n < 0 || (n > 0 && (!Y || !f_out))) return fail(BOSS_E_INVALID, "NULL argument");
    const FitProg& g = fit->g;
    double v[FIT_MAXI], av[FIT_MAXI];
    for (int j = 0; j < n; ++j) {
        const double* y = Y + (size_t)j * g.P;
        f_out[j] = fit_eval(g, y, v, 1);
        if (df_out) fit_grad(g, y, v, df_out + (size_t)j * g.P, av, 1);
    }
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// launches (declared in bosship.hip for host_predict.inc / host_acq.inc)
// ------------------------------------------------------------------------------------------
// What every Monte-Carlo entry point checks before any device work.
static int mc_check(const boss_fit_t* fit, int P, int S, int n_eps, const double* eps) {
    if (!fit || !eps) return fail(BOSS_E_INVALID, "NULL fitness program or eps");
    if (fit->g.P != P) return fail(BOSS_E_INVALID, "the fitness program takes " + std::to_string(fit->g.P) + " inputs, the call has P = " + std::to_string(P));
    if (n_eps < 1) return fail(BOSS_E_INVALID, "n_eps must be >= 1");
    if (S > 1 && n_eps != S) return fail(BOSS_E_INVALID, "S > 1 posterior samples take one eps column each: n_eps must equal S");
    if ((long long)P * n_eps > (1LL << 20)) return fail(BOSS_E_INVALID, "P*n_eps above 2^20 is not supported");
    for (size_t i = 0; i < (size_t)P * n_eps; ++i)
        if (!std::isfinite(eps[i])) return fail(BOSS_E_INVALID, "eps must be finite");
    return BOSS_OK;
}

// ε onto the device, once per call (the program itself travels in the kernel arguments)
static int mc_stage(Ctx* c, hipStream_t s, int P, const McEpi& mc, const double** deps_out) {
    const size_t bytes = sizeof(double) * (size_t)P * mc.n_eps;
    int rc = ws_reserve(c->mceps, bytes);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->mceps.p, mc.eps, bytes, hipMemcpyHostToDevice, s));
    *deps_out = (const double*)c->mceps.p;
    return BOSS_OK;
}

// workgroup size (whole waves, one candidate each) and dynamic LDS for a program: as many of the 4 waves as fit 64 KiB
static int mc_block(const FitProg& g, bool grad, size_t* lds) {
    const size_t per_wave = sizeof(double) * 64 * (size_t)mc_slots(g.P, g.nI, grad);
    const int waves = (int)std::max<size_t>(1, std::min<size_t>(MC_MAX_WAVES, (64 * 1024) / per_wave));
    *lds = per_wave * waves;
    return waves;
}

static void mc_accumulate_launch(hipStream_t s, const double* mu, const double* var, size_t sstride, int ldm, int M, int s0, int s1, int S_total,
                                 const EiPar& par, const McEpi& mc, const double* deps, double* acq_sum, int add) {
    size_t lds;
    const int waves = mc_block(*mc.g, false, &lds);
    hipLaunchKernelGGL(ei_mc_accumulate_kernel, dim3((M + waves - 1) / waves), dim3(64 * waves), lds, s, mu, var, sstride, ldm, M, s0, s1, S_total,
                       par, *mc.g, deps, mc.n_eps, acq_sum, add);
}

static void mc_grad_launch(hipStream_t s, const double* mu, const double* var, const double* dmu, const double* dvar, int M, int d, int S,
                           const EiPar& par, const McEpi& mc, const double* deps, const unsigned char* mask, double* acq, double* dacq) {
    size_t lds;
    const int waves = mc_block(*mc.g, true, &lds);
    hipLaunchKernelGGL(ei_mc_grad_set_kernel, dim3((M + waves - 1) / waves), dim3(64 * waves), lds, s, mu, var, dmu, dvar, M, d, S, par, *mc.g,
                       deps, mc.n_eps, mask, acq, dacq);
}

// ------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------
extern "C" int boss_acq_ei_mc(int P, int S, boss_gp_t* const* gps, const boss_cand_t* cand, const double* mean_Xs, const boss_fit_t* fit,
                              int n_eps, const double* eps, const double* y_max, int has_best, double best,
                              const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    if (P < 1 || S < 1) return fail(BOSS_E_INVALID, "bad arguments");
    int rc = mc_check(fit, P, S, n_eps, eps);
    if (rc) return rc;
    const McEpi mc{&fit->g, n_eps, eps};
    return acq_ei_impl(P, S, gps, cand, mean_Xs, nullptr, y_max, has_best, best, valid_mask, acq_out, argmax_out, max_out, nullptr, 0, false, &mc);
}

extern "C" int boss_acq_ei_mc_grad(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                   const double* mean_grad, const boss_fit_t* fit, int n_eps, const double* eps, const double* y_max,
                                   int has_best, double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    if (P < 1 || S < 1) return fail(BOSS_E_INVALID, "bad arguments");
    int rc = mc_check(fit, P, S, n_eps, eps);
    if (rc) return rc;
    const McEpi mc{&fit->g, n_eps, eps};
    return acq_ei_grad_set_impl(P, S, gps, M, Xs, mean_Xs, mean_grad, nullptr, y_max, has_best, best, valid_mask, acq_out, dacq_out, &mc);
}

// From moments on the host: mu / var S×P×M as boss_acq_ei_moments takes them.
extern "C" int boss_acq_ei_mc_moments(int device, int P, int S, int M, const double* mu, const double* var, const boss_fit_t* fit, int n_eps,
                                      const double* eps, const double* y_max, int has_best, double best,
                                      const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    if (P < 1 || S < 1 || M < 1 || !mu || !var) return fail(BOSS_E_INVALID, "bad arguments");
    int rc = mc_check(fit, P, S, n_eps, eps);
    if (rc) return rc;
    if ((long long)P * S * M > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M above 2^30 is not supported");
    const McEpi mc{&fit->g, n_eps, eps};
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
    rc = ei_params(c, s, P, no_coefs, y_max, has_best, best, &par, nullptr, nullptr);   // (P <= EI_MAXP: by value)
    if (rc) return rc;
    const double* deps = nullptr;
    rc = mc_stage(c, s, P, mc, &deps);
    if (rc) return rc;
    (void)hipMemcpyAsync(dmu, mu, sizeof(double) * pm * S, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(dvar, var, sizeof(double) * pm * S, hipMemcpyHostToDevice, s);
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    ei_value_epilogue_launch(s, dmu, dvar, M, S, par, nullptr, nullptr, valid_mask ? dmask : nullptr, &mc, deps, dacq, hres, 0ull);
    if (acq_out) (void)hipMemcpyAsync(acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    hipError_t e2 = hipGetLastError();
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    if (e2 != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e2));
    if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
    if (max_out) *max_out = hres[0];
    return BOSS_OK;
}

// From moments and moment gradients on the host: mu / var [s][p][M], dmu / dvar [s][p][d×M] (boss_acq_ei_grad_moments with a leading S).
extern "C" int boss_acq_ei_mc_grad_moments(int device, int P, int S, int M, int d, const double* mu, const double* var, const double* dmu,
                                           const double* dvar, const boss_fit_t* fit, int n_eps, const double* eps, const double* y_max,
                                           int has_best, double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out) {
    if (P < 1 || S < 1 || M < 1 || d < 1 || !mu || !var || !dmu || !dvar || !acq_out || !dacq_out) return fail(BOSS_E_INVALID, "bad arguments");
    int rc = mc_check(fit, P, S, n_eps, eps);
    if (rc) return rc;
    if ((long long)P * S * M * d > (1LL << 30)) return fail(BOSS_E_INVALID, "P·S·M·d above 2^30 is not supported");
    const McEpi mc{&fit->g, n_eps, eps};
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
    EiPar par;
    const double no_coefs[EI_MAXP] = {};
    rc = ei_params(c, s, P, no_coefs, y_max, has_best, best, &par, nullptr, nullptr);
    if (rc) return drain(c, rc);
    const double* deps = nullptr;
    rc = mc_stage(c, s, P, mc, &deps);
    if (rc) return drain(c, rc);
    (void)hipMemcpyAsync(d_mu, mu, sizeof(double) * nm, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_var, var, sizeof(double) * nm, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_gm, dmu, sizeof(double) * ndm, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(d_gv, dvar, sizeof(double) * ndm, hipMemcpyHostToDevice, s);
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    ei_grad_epilogue_launch(s, d_mu, d_var, d_gm, d_gv, M, d, S, false, par, nullptr, nullptr, valid_mask ? dmask : nullptr, &mc, deps, dacq, ddacq);
    return finish(c, {{acq_out, dacq, sizeof(double) * M}, {dacq_out, ddacq, sizeof(double) * dm}});
}
