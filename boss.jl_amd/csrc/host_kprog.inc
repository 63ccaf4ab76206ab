// host_kprog.inc — kernel programs (boss_kern_t) and the posteriors built on them (boss_kgp_create): validation, the host
// interpreter, the launches factor_enqueue / predict_enqueue / predict_set_enqueue make for such handles, and the batched entry
// points boss_kgp_loglike_batch / boss_kgp_fit_batch on the hooks of host_batch.inc (included by bosship.hip, behind host_batch.inc).

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
    int rc = fit_build(2 * d, n_const, consts, n_instr, code, out_id, "", "kernel", FIT_NOPS, &g);
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

// Appends and tracked candidates on (on != 0) or off for a program-kernel posterior: boss_gp_append, boss_gp_reserve and
// boss_track_create (and with it boss_track_sync / _moments / _free, boss_acq_ei_tracks) take the handle while the flag is set.
// Before or after boss_gp_update; nothing resident changes; independent of boss_kgp_set_grad.
extern "C" int boss_kgp_set_sequential(boss_gp_t* g, int on) {
    if (!g) return fail(BOSS_E_INVALID, "gp is NULL");
    if (!g->kprog) return fail(BOSS_E_INVALID, "handle was not created by boss_kgp_create");
    std::lock_guard<std::mutex> lk(g->ctx->mtx);
    g->kseq = on != 0;
    return BOSS_OK;
}

// ------------------------------------------------------------------------------------------
// launches (declared in bosship.hip for host_factor.inc / host_append.inc / host_predict.inc / host_track.inc)
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
    hipLaunchKernelGGL(kprog_gram_kernel, dim3(t64 * (t64 + 1) / 2, 1, 1), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, (size_t)0, g->d,
                       g->N, g->Np, (const double*)g->hyp, (size_t)0, g->A, g->ld, (size_t)0, 0);
}

// ... of block row kb alone (append_rows_enqueue): its 4·kb + 3 tiles of 64×64 from triangular tile index kb (2 kb + 1), the
// built-in kernels' numbers; g->N counts the new observations, rows behind them are those of the identity
static void kprog_gram_rows_launch(boss_gp* g, int kb, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(*g->kp, g->d, &lds);
    hipLaunchKernelGGL(kprog_gram_kernel, dim3(4 * kb + 3, 1, 1), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, (size_t)0, g->d, g->N,
                       g->Np, (const double*)g->hyp, (size_t)0, g->A, g->ld, (size_t)0, kb * (2 * kb + 1));
}

// ... of cnt parameter sets with constant strides (boss_kgp_loglike_batch, boss_kgp_fit_batch): the sets' scaled points from the
// shared raw points and their 1/λ (par, sPar apart), then all Gram matrices in one launch (grid.z = set; hyp = {α², σ²} per set)
static void kprog_gram_batch_launch(const FitProg& kp, int d, int N, int Np, int cnt, const double* Xraw, const double* par, size_t sPar,
                                    const double* hyp, size_t sHyp, double* Xsc, size_t sX, double* A, int ld, size_t bstride, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(kp, d, &lds);
    const int t64 = Np / 64;
    hipLaunchKernelGGL(kprog_scale_set_kernel, dim3((Np + 255) / 256, cnt), dim3(256), 0, s, Xraw, Xsc, sX, par, sPar, d, Np);
    hipLaunchKernelGGL(kprog_gram_kernel, dim3(t64 * (t64 + 1) / 2, 1, cnt), dim3(threads), lds, s, kp, (const double*)Xsc, sX, d, N, Np, hyp,
                       sHyp, A, ld, bstride, 0);
}

// K* of `tiles` candidate tiles of BN (32 or 64) into out[tile][Np][BN], and k(x*, x*) of their candidates into pvar
static void kprog_kstar_launch(boss_gp* g, const boss_cand* cd, const double* Csc, int BN, int tiles, double* out, double* pvar, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(*g->kp, g->d, &lds);
    auto kfn = BN == 32 ? kprog_kstar_kernel<32> : kprog_kstar_kernel<64>;
    hipLaunchKernelGGL(kfn, dim3(g->Np / 256, tiles), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, g->d, g->N, g->Np, Csc, cd->Mp,
                       cd->M, g->amp2, out, pvar);
}

// The new column of a rank-one append (append_locked): R[row][0] = (α+1e-8)² f(u_row, u_new) for the N0 old rows in column 0 of a
// 32-wide tile (the layout kstar_rows_kernel writes there; 0 for the rows behind them), and kself[0] = (α+1e-8)² f(u_new, u_new), the
// prior variance the new diagonal entry starts from.  Csc: the new scaled point as candidate 0 of a 64-wide candidate block.
static void kprog_append_col_launch(boss_gp* g, int N0, const double* Csc, double* R, double* kself, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(*g->kp, g->d, &lds);
    hipLaunchKernelGGL(kprog_col_kernel, dim3((g->Np + threads - 1) / threads), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, g->d, N0,
                       g->Np, Csc, 64, g->amp2, R, kself);
}

// the right-hand sides of the n <= TRACK_ROWS rows from N0 on for `tiles` candidate tiles of a track (track_sync_locked)
static void kprog_track_rhs_launch(boss_gp* g, int N0, int n, const double* Csc, int Mp, int M, int tiles, double* rhs, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(*g->kp, g->d, &lds);
    hipLaunchKernelGGL(kprog_track_rhs_kernel, dim3(tiles), dim3(threads), lds, s, *g->kp, (const double*)g->Xsc, g->d, g->Np, N0, n, Csc, Mp, M,
                       g->amp2, rhs);
}

static void kprog_var_launch(hipStream_t s, double* var, const double* pvar, int M) {
    hipLaunchKernelGGL(kprog_var_kernel, dim3((M + 255) / 256), dim3(256), 0, s, var, pvar, M);
}

// K* of cnt members of a set (descriptors dsets, one program, one shape: predict_set_ok) into their V slabs of 32 candidates, their
// prior variances into pvar (spv apart); and the σ² of the set behind predict_kernel_set<G, true> (predict_set_enqueue)
static void kprog_kstar_set_launch(boss_gp* g0, const boss_cand* cd, const PredSet* dsets, int tiles, int cnt, double* V, double* pvar,
                                   size_t spv, hipStream_t s) {
    size_t lds;
    const int threads = kprog_block(*g0->kp, g0->d, &lds);
    hipLaunchKernelGGL(kprog_kstar_set_kernel, dim3(g0->Np / 256, tiles, cnt), dim3(threads), lds, s, *g0->kp, g0->d, g0->N, g0->Np, cd->Mp,
                       cd->M, dsets, V, pvar, spv);
}
static void kprog_var_set_launch(hipStream_t s, const PredSet* dsets, int cnt, const double* pvar, size_t spv, int M) {
    hipLaunchKernelGGL(kprog_var_set_kernel, dim3((M + 255) / 256, cnt), dim3(256), 0, s, dsets, pvar, spv, M);
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

// ------------------------------------------------------------------------------------------
// S hyper-parameter sets of one output slice under one program (boss_kgp_loglike_batch, boss_kgp_fit_batch): `loglike.(samples)` of
// src/model_fitters/sampling.jl:59-78 and the S posteriors of a Bayesian-inference fit (src/posterior.jl:15-19) for a
// KernelFunctions.Kernel beyond the built-in ones.  The fourth model on the hooks of host_batch.inc: the parameter block of a set is
// [1/λ (d) | α², σ²] as stage_hyper leaves it (the resident block of a handle), the Gram hook scales the shared points per set and
// launches kprog_gram_kernel over all sets of the chunk (kprog_gram_batch_launch).
// ------------------------------------------------------------------------------------------
static int kgp_batch_args(const boss_kern_t* kern, int d, int N, int S, const double* X, const double* y) {
    if (!kern) return fail(BOSS_E_INVALID, "kern is NULL");
    if (d != kern->d)
        return fail(BOSS_E_INVALID, "the kernel program was created for x_dim = " + std::to_string(kern->d) + ", the call has d = " + std::to_string(d));
    if (S < 0) return fail(BOSS_E_INVALID, "S must be >= 0");
    if (N < 1 || !X || !y) return fail(BOSS_E_INVALID, "need N >= 1 and non-NULL X, y");
    if (N > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");
    return BOSS_OK;
}

extern "C" int boss_kgp_loglike_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                                      const boss_kern_t* kern, int S, const double* lengthscales, const double* amplitudes,
                                      const double* noise_stds, const double* mean_X, int mean_stride, double* ll_out, int* status_out) {
    int rc = kgp_batch_args(kern, d, N, S, X, y);
    if (rc) return rc;
    if (S == 0) return BOSS_OK;
    if (!ll_out) return fail(BOSS_E_INVALID, "ll_out is NULL");
    if (!lengthscales || !amplitudes || !noise_stds) return fail(BOSS_E_INVALID, "NULL hyper-parameter array");
    if (mean_X && mean_stride != 0 && mean_stride != N) return fail(BOSS_E_INVALID, "mean_stride must be 0 or N");
    Ctx* c;
    rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mtx);
    const int Np = round_up(N, BLK);
    std::vector<double> pts, yb(Np, 0.0);
    pack_points(pts, X, d, N, Np, discrete);
    std::copy(y, y + N, yb.begin());
    const size_t par_doubles = (size_t)d + 2, sX = (size_t)d * Np, bstride = (size_t)(Np + RHS_ROWS) * Np;
    // the scaled points of a chunk's sets, [set][d][Np] (the chunk is model_loglike_batch_run's: its matrices below batch_chunk_bytes)
    const size_t chunk = std::max<size_t>(1, std::min<size_t>((size_t)S, batch_chunk_bytes() / (bstride * sizeof(double))));
    rc = ws_reserve(c->kxs, sizeof(double) * sX * chunk);
    if (rc) return rc;
    auto fill = [&](int b, double* p) { return stage_hyper(d, lengthscales + (size_t)b * d, amplitudes[b], noise_stds[b], p, p + d); };
    auto gram = [&](const ModelBatchGramArgs& a) {
        const size_t b0 = (size_t)(a.A - (double*)c->batchA.p) / a.bstride;   // (first set of this launch within the chunk)
        kprog_gram_batch_launch(kern->g, d, N, Np, a.cnt, a.pts, a.par, par_doubles, a.par + d, par_doubles, (double*)c->kxs.p + b0 * sX, sX, a.A,
                                a.ld, a.bstride, c->stream);
    };
    return model_loglike_batch_run(c, N, Np, S, pts, yb, mean_X, mean_stride, par_doubles, fill, gram, ll_out, status_out);
}

// The S posteriors as resident handles out of one batched factorisation: members of one slab as boss_gp_fit_batch's, each a program
// handle (kprog, KERN_PROGRAM, its own copy of the program) — whatever takes or refuses a boss_kgp_create handle treats a member alike.
extern "C" int boss_kgp_fit_batch(int device, const boss_kern_t* kern, int d, int N, const double* X, const double* y, const double* mean_X,
                                  int mean_stride, const unsigned char* discrete, int S, const double* lengthscales,
                                  const double* amplitudes, const double* noise_stds, boss_gp_t** out, double* logpdf_out, int* status_out) {
    if (out)
        for (int b = 0; b < S; ++b) out[b] = nullptr;
    int rc = kgp_batch_args(kern, d, N, S, X, y);
    if (rc) return rc;
    if (S == 0) return BOSS_OK;
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    if (!lengthscales || !amplitudes || !noise_stds) return fail(BOSS_E_INVALID, "NULL hyper-parameter array");
    if (mean_X && mean_stride != 0 && mean_stride != N) return fail(BOSS_E_INVALID, "mean_stride must be 0 or N");
    Ctx* c;
    rc = get_ctx(device, &c);
    if (rc) return rc;
    const int Np = round_up(N, PRED_RB);
    std::vector<double> pts, yb(Np, 0.0), h_par;
    std::vector<int> valid(S);
    pack_points(pts, X, d, N, Np, discrete);
    std::copy(y, y + N, yb.begin());
    FitBatchSpec sp;
    sp.kernel = KERN_PROGRAM;
    sp.d = d;
    sp.N = sp.npts = N;
    sp.ldx = Np;
    sp.S = S;
    sp.pts = &pts;
    sp.yb = &yb;
    sp.mean_X = mean_X;
    sp.mean_stride = mean_stride;
    sp.discrete = discrete;
    auto factor = [&](FitBatchSlab& L, hipStream_t s) {
        h_par.assign(L.sPar * S, 0.0);                       // the members' own blocks [1/λ (d) | α², σ², -, -], uploaded in place
        for (int b = 0; b < S; ++b) {
            double* p = &h_par[(size_t)b * L.sPar];
            valid[b] = stage_hyper(d, lengthscales + (size_t)b * d, amplitudes[b], noise_stds[b], p, p + d);
        }
        hipError_t e = hipMemcpyAsync(L.par, h_par.data(), sizeof(double) * L.sPar * S, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        batch_middle_enqueue(c, N, Np, S, L.y, (const double*)L.mean, L.sMean, L.A, L.ld, L.sA, L.inv16, L.sInv, L.scalB, L.infoB, BatchStage(),
                             [&](int b0, int cnt) {
                                 ProfScope ps(c, "gram");
                                 const double* par = L.par + (size_t)b0 * L.sPar;
                                 kprog_gram_batch_launch(kern->g, d, N, Np, cnt, L.pts, par, L.sPar, par + d, L.sPar, L.Xsc + (size_t)b0 * L.sX, L.sX,
                                                         L.A + (size_t)b0 * L.sA, L.ld, L.sA, c->stream);
                             });
        return hipSuccess;
    };
    auto member = [&](int b, boss_gp* g) {
        const double* p = &h_par[(size_t)b * round_up(d + 4, 8)];
        for (int k = 0; k < d + 2; ++k) g->host_par[k] = p[k];
        g->amp2 = p[d];
        g->kprog = true;
        g->kp = new FitProg(kern->g);
        return valid[b] != 0;
    };
    return fit_batch_run(c, sp, factor, member, out, logpdf_out, status_out);
}
