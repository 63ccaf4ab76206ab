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
