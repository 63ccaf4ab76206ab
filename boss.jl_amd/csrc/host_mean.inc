// host_mean.inc — mean programs (boss_mean_t): the handle, the host interpreter and the device call (included by bosship.hip).

struct boss_mean {
    int d = 0, T = 0, P = 0, nI_max = 0;
    std::vector<FitProg> g;                                  // one program per output, each over the d + T shared inputs
};

// ------------------------------------------------------------------------------------------
// the handle: validation only, no device
// ------------------------------------------------------------------------------------------
extern "C" int boss_mean_create(int d, int T, int P, const int* n_const, const double* consts, const int* n_instr, const int* code,
                                const int* out_ids, boss_mean_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || T < 0 || d + T > MEAN_MAXIN) return fail(BOSS_E_INVALID, "a mean program takes d >= 1 and T >= 0 with d + T <= 32 inputs");
    if (P < 1 || P > EI_MAXP) return fail(BOSS_E_INVALID, "a mean program has 1 to 16 outputs");
    if (!n_const || !n_instr || !out_ids) return fail(BOSS_E_INVALID, "NULL n_const, n_instr or out_ids");
    boss_mean* mp = new boss_mean();
    mp->d = d;
    mp->T = T;
    mp->P = P;
    mp->g.resize(P);
    const double* c = consts;
    const int* k = code;
    for (int p = 0; p < P; ++p) {
        int rc = fit_build(d + T, n_const[p], c, n_instr[p], k, out_ids[p], "output " + std::to_string(p) + ": ", "mean", FIT_NOPS, &mp->g[p]);
        if (rc) {
            delete mp;
            return rc;
        }
        c += n_const[p];                                     // (both counts passed fit_build: within 0..32 and 0..64)
        k += 3 * (size_t)n_instr[p];
        mp->nI_max = std::max(mp->nI_max, n_instr[p]);
    }
    *out = mp;
    return BOSS_OK;
}

extern "C" void boss_mean_free(boss_mean_t* mp) { delete mp; }

// What both evaluation calls check before any work.
static int mean_check(const boss_mean_t* mp, int n, const double* X, int S, const double* thetas, int layout, const double* m,
                      const double* jac_theta) {
    if (!mp) return fail(BOSS_E_INVALID, "NULL mean program");
    if (n < 1 || S < 1) return fail(BOSS_E_INVALID, "n and S must be >= 1");
    if (!X || !m) return fail(BOSS_E_INVALID, "NULL X or m");
    if (mp->T > 0 && !thetas) return fail(BOSS_E_INVALID, "thetas is NULL, the mean program takes T = " + std::to_string(mp->T) + " parameters");
    if (mp->T == 0 && jac_theta) return fail(BOSS_E_INVALID, "jac_theta asked of a mean program without parameters (T = 0)");
    if (layout != 0 && layout != 1) return fail(BOSS_E_INVALID, "layout must be 0 (sample-major) or 1 (output-major)");
    const long long w = std::max(1, std::max(mp->T, mp->d));
    if ((long long)mp->P * S > (1LL << 30) || (long long)mp->P * S * n > (1LL << 30) || (long long)mp->P * S * n * w > (1LL << 30))
        return fail(BOSS_E_INVALID, "P·S·n·max(1, T, d) above 2^30 is not supported");
    return BOSS_OK;
}

// The kernel's loop on the host (tests, no device): the same fit_eval / fit_grad on unit-stride columns.
extern "C" int boss_mean_eval_host(const boss_mean_t* mp, int n, const double* X, int S, const double* thetas, int layout, double* m,
                                   double* jac_theta, double* jac_x) {
    int rc = mean_check(mp, n, X, S, thetas, layout, m, jac_theta);
    if (rc) return rc;
    const int d = mp->d, T = mp->T, P = mp->P;
    double y[MEAN_MAXIN], ay[MEAN_MAXIN], v[FIT_MAXI], av[FIT_MAXI];
    for (int s = 0; s < S; ++s)
        for (int p = 0; p < P; ++p) {
            const FitProg& g = mp->g[p];
            const size_t blk = mean_block(layout, p, s, P, S);
            for (int t = 0; t < T; ++t) y[d + t] = thetas[(size_t)s * T + t];
            for (int j = 0; j < n; ++j) {
                for (int k = 0; k < d; ++k) y[k] = X[(size_t)j * d + k];
                m[blk * n + j] = fit_eval(g, y, v, 1);
                if (!jac_theta && !jac_x) continue;
                fit_grad(g, y, v, ay, av, 1);
                if (jac_theta)
                    for (int t = 0; t < T; ++t) jac_theta[blk * n * T + (size_t)t * n + j] = ay[d + t];
                if (jac_x)
                    for (int k = 0; k < d; ++k) jac_x[blk * n * d + (size_t)j * d + k] = ay[k];
            }
        }
    return BOSS_OK;
}

// workgroup size (whole waves, one point per thread) and dynamic LDS for a program: as many of the 4 waves as fit 64 KiB, and no more
// than the points need
static int mean_waves(const boss_mean* mp, bool grad, int n, size_t* lds) {
    const size_t per_wave = sizeof(double) * 64 * (size_t)std::max(1, mean_slots(mp->d + mp->T, mp->nI_max, grad));
    int waves = (int)std::max<size_t>(1, std::min<size_t>(MEAN_MAX_WAVES, (64 * 1024) / per_wave));
    waves = std::max(1, std::min(waves, (n + 63) / 64));
    *lds = per_wave * waves;
    return waves;
}

// (tests) the workgroup shape boss_mean_eval launches for n points: waves per workgroup; dynamic LDS bytes in *lds_out
extern "C" int boss_debug_mean_block(const boss_mean_t* mp, int grad, int n, int* lds_out) {
    if (!mp || n < 1) return 0;
    size_t lds;
    const int waves = mean_waves(mp, grad != 0, n, &lds);
    if (lds_out) *lds_out = (int)lds;
    return waves;
}

extern "C" int boss_mean_eval(int device, const boss_mean_t* mp, int n, const double* X, int S, const double* thetas, int layout, double* m,
                              double* jac_theta, double* jac_x) {
    int rc = mean_check(mp, n, X, S, thetas, layout, m, jac_theta);
    if (rc) return rc;
    Ctx* c;
    rc = get_ctx(device, &c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const int d = mp->d, T = mp->T, P = mp->P;
    const bool grad = jac_theta || jac_x;
    const size_t nb = (size_t)P * S * n;                     // values; the Jacobians T and d times that
    const size_t n_m = nb, n_jt = jac_theta ? nb * T : 0, n_jx = jac_x ? nb * d : 0;
    const size_t n_x = (size_t)d * n, n_th = (size_t)T * S;
    const size_t prog_bytes = sizeof(FitProg) * (size_t)P;   // (a multiple of 8)
    // programs | X | thetas | m | jac_theta | jac_x
    rc = ws_reserve(c->meanws, prog_bytes + sizeof(double) * (n_x + n_th + n_m + n_jt + n_jx));
    if (rc) return rc;
    FitProg* dprogs = (FitProg*)c->meanws.p;
    double* dX = (double*)((char*)c->meanws.p + prog_bytes);
    double* dth = dX + n_x;
    double* dm = dth + n_th;
    double* djt = dm + n_m;
    double* djx = djt + n_jt;
    (void)hipMemcpyAsync(dprogs, mp->g.data(), prog_bytes, hipMemcpyHostToDevice, s);
    (void)hipMemcpyAsync(dX, X, sizeof(double) * n_x, hipMemcpyHostToDevice, s);
    if (T > 0) (void)hipMemcpyAsync(dth, thetas, sizeof(double) * n_th, hipMemcpyHostToDevice, s);
    size_t lds;
    const int waves = mean_waves(mp, grad, n, &lds);
    const dim3 grid((n + 64 * waves - 1) / (64 * waves), P, std::min(S, 65535)), block(64 * waves);
    if (grad)
        hipLaunchKernelGGL(mean_eval_kernel<true>, grid, block, lds, s, (const FitProg*)dprogs, (const double*)dX, (const double*)dth, n, d, T,
                           P, S, layout, mp->nI_max, dm, jac_theta ? djt : nullptr, jac_x ? djx : nullptr);
    else
        hipLaunchKernelGGL(mean_eval_kernel<false>, grid, block, lds, s, (const FitProg*)dprogs, (const double*)dX, (const double*)dth, n, d, T,
                           P, S, layout, mp->nI_max, dm, (double*)nullptr, (double*)nullptr);
    // m | jac_theta | jac_x lie together: one copy through the pinned area where they fit it, one copy each otherwise
    const size_t total = sizeof(double) * (n_m + n_jt + n_jx);
    hipError_t e;
    if (total <= PINNED_DOWN_BYTES) {
        char* stage = (char*)c->pinned + PINNED_DOWN_OFF;
        (void)hipMemcpyAsync(stage, dm, total, hipMemcpyDeviceToHost, s);
        e = hipStreamSynchronize(s);
        std::memcpy(m, stage, sizeof(double) * n_m);
        if (jac_theta) std::memcpy(jac_theta, stage + sizeof(double) * n_m, sizeof(double) * n_jt);
        if (jac_x) std::memcpy(jac_x, stage + sizeof(double) * (n_m + n_jt), sizeof(double) * n_jx);
    } else {
        (void)hipMemcpyAsync(m, dm, sizeof(double) * n_m, hipMemcpyDeviceToHost, s);
        if (jac_theta) (void)hipMemcpyAsync(jac_theta, djt, sizeof(double) * n_jt, hipMemcpyDeviceToHost, s);
        if (jac_x) (void)hipMemcpyAsync(jac_x, djx, sizeof(double) * n_jx, hipMemcpyDeviceToHost, s);
        e = hipStreamSynchronize(s);
    }
    const hipError_t e2 = hipGetLastError();                 // (read either way: it also clears the error)
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    return BOSS_OK;
}
