// host_kprog.inc — kernel programs (boss_kern_t) and the posteriors built on them (boss_kgp_create): validation, the host
// interpreter, and the launches factor_enqueue / predict_enqueue make for such a handle (included by bosship.hip).

struct boss_kern {
    FitProg g;                                               // 2·d inputs: u[0..d) then v[0..d)
    int d;
};

// ------------------------------------------------------------------------------------------
// the program: validation only, no device
// ------------------------------------------------------------------------------------------
extern "C" int boss_kern_create(int d, int n_const, const double* consts, int n_instr, const int* code, int out_id, boss_kern_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || d > KPROG_MAX_D) return fail(BOSS_E_INVALID, "a kernel program takes two points of 1 to 16 dimensions");
    FitProg g;
    int rc = fit_build(2 * d, n_const, consts, n_instr, code, out_id, "", "kernel", &g);
    if (rc) return rc;
    boss_kern* k = new boss_kern();
    k->g = g;
    k->d = d;
    *out = k;
    return BOSS_OK;
}

extern "C" void boss_kern_free(boss_kern_t* kern) { delete kern; }

extern "C" int boss_kern_eval_host(const boss_kern_t* kern, int n, const double* U, const double* V, double* k_out) {
    if (!kern || n < 0 || (n > 0 && (!U || !V || !k_out))) return fail(BOSS_E_INVALID, "NULL argument");
    const int d = kern->d;
    double y[2 * KPROG_MAX_D], v[FIT_MAXI];
    for (int j = 0; j < n; ++j) {
        for (int k = 0; k < d; ++k) {
            y[k] = U[(size_t)j * d + k];
            y[d + k] = V[(size_t)j * d + k];
        }
        k_out[j] = fit_eval(kern->g, y, v, 1);
    }
    return BOSS_OK;
}

// k and all 2d partials of n pairs: dU[j·d + m] = ∂f/∂u_m, dV[j·d + m] = ∂f/∂v_m at (U[:, j], V[:, j]) — the reverse sweep the gradient
// kernels run (kern_grad, fitness.hpp), with its convention that a local partial of exactly 0 passes 0 on.  k_out may be NULL.
extern "C" int boss_kern_grad_host(const boss_kern_t* kern, int n, const double* U, const double* V, double* k_out, double* dU, double* dV) {
    if (!kern || n < 0 || (n > 0 && (!U || !V || !dU || !dV))) return fail(BOSS_E_INVALID, "NULL argument");
    const int d = kern->d;
    double y[2 * KPROG_MAX_D], v[FIT_MAXI], ay[2 * KPROG_MAX_D], av[FIT_MAXI];
    for (int j = 0; j < n; ++j) {
        for (int k = 0; k < d; ++k) {
            y[k] = U[(size_t)j * d + k];
            y[d + k] = V[(size_t)j * d + k];
        }
        const double f = fit_eval(kern->g, y, v, 1);
        kern_grad(kern->g, y, v, ay, av, 1);
        if (k_out) k_out[j] = f;
        for (int k = 0; k < d; ++k) {
            dU[(size_t)j * d + k] = ay[k];
            dV[(size_t)j * d + k] = ay[d + k];
        }
    }
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// the posterior handle: a plain handle's storage, its kernel id replaced by the program
// ------------------------------------------------------------------------------------------
extern "C" int boss_kgp_create(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                               const boss_kern_t* kern, boss_gp_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!kern) return fail(BOSS_E_INVALID, "kern is NULL");
    if (d != kern->d)
        return fail(BOSS_E_INVALID, "the kernel program was created for x_dim = " + std::to_string(kern->d) + ", the call has d = " + std::to_string(d));
    int rc = gp_create_common(device, KERN_SQEXP, d, N, N, X, y, discrete, false, out);   // (the id is replaced below)
    if (rc) return rc;
    boss_gp* g = *out;
    g->kprog = true;
    g->kernel = KERN_PROGRAM;
    g->kp = new FitProg(kern->g);
    return BOSS_OK;
}

// Gradients on (on != 0) or off for a program-kernel posterior: boss_gp_loglike_grad[_mean], boss_gp_predict_grad and
// boss_acq_ei_grad[_set] take the handle while the flag is set.  Before or after boss_gp_update; nothing resident changes.
extern "C" int boss_kgp_set_grad(boss_gp_t* g, int on) {
    if (!g) return fail(BOSS_E_INVALID, "gp is NULL");
    if (!g->kprog) return fail(BOSS_E_INVALID, "handle was not created by boss_kgp_create");
    std::lock_guard<std::mutex> lk(g->ctx->mtx);
    g->kgrad = on != 0;
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// launches (declared in bosship.hip for host_factor.inc / host_predict.inc)
// ------------------------------------------------------------------------------------------
// workgroup size (whole waves) and dynamic LDS of a program over d dimensions: as many of the 4 waves as fit 64 KiB
static int kprog_block(const FitProg& g, int d, size_t* lds) {
    const size_t per_wave = sizeof(double) * 64 * (size_t)kprog_slots(d, g.nI);
    const int waves = (int)std::max<size_t>(1, std::min<size_t>(KPROG_MAX_WAVES, (64 * 1024) / per_wave));
    *lds = per_wave * waves;
    return 64 * waves;
}

// the Gram matrix of the handle's scaled points under its resident hyper-parameters into g->A
static void kprog_gram_launch(boss_gp* g, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(*g->kp, g->d, &lds);
    const int t64 = g->Np / 64;
    hipLaunchKernelGGL(kprog_gram_kernel, dim3(t64 * (t64 + 1) / 2), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, g->d, g->N, g->Np,
                       (const double*)g->hyp, g->A, g->ld);
}

// K* of `tiles` candidate tiles of BN (32 or 64) into out[tile][Np][BN], and k(x*, x*) of their candidates into pvar
static void kprog_kstar_launch(boss_gp* g, const boss_cand* cd, const double* Csc, int BN, int tiles, double* out, double* pvar, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(*g->kp, g->d, &lds);
    auto kfn = BN == 32 ? kprog_kstar_kernel<32> : kprog_kstar_kernel<64>;
    hipLaunchKernelGGL(kfn, dim3(g->Np / 256, tiles), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, g->d, g->N, g->Np, Csc, cd->Mp,
                       cd->M, g->amp2, out, pvar);
}

static void kprog_var_launch(hipStream_t s, double* var, const double* pvar, int M) {
    hipLaunchKernelGGL(kprog_var_kernel, dim3((M + 255) / 256), dim3(256), 0, s, var, pvar, M);
}

// ... of the gradient kernels: a column holds values and adjoints (kprog_grad_slots), at least min_slots doubles per thread
static int kprog_grad_block(const FitProg& g, int d, int min_slots, size_t* lds) {
    const size_t per_wave = sizeof(double) * 64 * (size_t)std::max(kprog_grad_slots(d, g.nI), min_slots);
    const int waves = (int)std::max<size_t>(1, std::min<size_t>(KPROG_MAX_WAVES, (64 * 1024) / per_wave));
    *lds = per_wave * waves;
    return 64 * waves;
}

// the per-tile Σ-vectors of the likelihood gradient (llgrad_enqueue, in llgrad_tile_kernel's place)
static void kprog_llgrad_launch(boss_gp* g, hipStream_t s, int ntiles, const double* Kinv, const double* apart, int nch, double* parts) {
    size_t lds;
    const int threads = kprog_grad_block(*g->kp, g->d, 0, &lds);
    hipLaunchKernelGGL(kprog_llgrad_tile_kernel, dim3(ntiles), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, g->d, g->N, g->Np,
                       (const double*)g->hyp, Kinv, g->ld, apart, nch, parts);
}

// ∇μ, ∇σ² behind the W slabs (grad_enqueue, in grad_accum_kernel's place); part: [tile][rsplit][2 (GRAD_MAX_D + 1)][32] for rsplit > 1
static void kprog_grad_accum_launch(boss_gp* g, const boss_cand* cd, hipStream_t s, int tiles, int rsplit, const double* slabs, const double* Csc,
                                    const double* mean_grad_dev, double* dmu, double* dvar, double* part) {
    size_t lds;
    const int threads = kprog_grad_block(*g->kp, g->d, 2 * (GRAD_MAX_D + 1), &lds);   // (the columns' LDS also takes the row subsets' sums)
    hipLaunchKernelGGL(kprog_grad_accum_kernel, dim3(tiles, rsplit), dim3(threads), lds, s, *g->kp, slabs, (const double*)g->avec, g->Np, g->N,
                       (const double*)g->Xsc, Csc, g->d, cd->Mp, cd->M, g->amp2, (const double*)g->invlam,
                       (const unsigned char*)g->discrete_dev, mean_grad_dev, dmu, dvar, part);
}
