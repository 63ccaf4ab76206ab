// host_batch.inc — boss_gp_loglike_batch, boss_ggp_loglike_batch, boss_ngp_loglike_batch and their _grad_batch forms, boss_gp_fit_batch, boss_ggp_fit_batch,
// boss_ngp_fit_batch: S hyper-parameter sets on one data slice (included by bosship.hip).  boss_kgp_loglike_batch and boss_kgp_fit_batch
// (host_kprog.inc) run on the same hooks.

// ------------------------------------------------------------------------------------------
// batched log-likelihood
// ------------------------------------------------------------------------------------------
static int llgrad_enqueue(boss_gp* g, hipStream_t s, double* sums_out, int bank, const SetBatch& B, const double* amp2_dev,
                          int amp2_stride, const MeanFold* mf = nullptr);
static void llgrad_finalize(int d, int N, const double* invlam, double amp2, double sig2, double zz, const double* h, double* grad_out);
static void ggp_llgrad_finalize(int d, const double* hp, const double* h, double* grad_out);

// Scaled points, right-hand sides, Gram matrices, factors and log-determinants of nb hyper-parameter sets laid out with constant strides
// (shared by boss_gp_loglike_batch and boss_gp_fit_batch).  Replaces the S likelihood / posterior evaluations of
// /root/reference/src/model_fitters/sampling.jl:59-78 and src/posterior.jl:15-19.  Caller holds the context lock; the work is complete
// on c->stream's timeline when the function returns.
// BOSS_BATCH_CHUNK_MB=<MB> (off by default) sends the sets through in chunks whose matrices fit the Infinity Cache together, dealt to up
// to BOSS_BATCH_STREAMS (3) streams.  Measured at BASELINE config 5 (512 × N = 1024, round 4): 14.2 ms with 192 MB chunks on three
// streams against 6.5-6.9 ms in one batch — a chunk costs the same ≈ 50 launches as the whole batch, and 25 chunks make the call
// launch-bound on the host.  Where the one batch spends its 6.6 ms (rocprofv3, per call): trailing updates 3.0 ms (K = 256 tiles at
// 48 TFLOP/s, 3.5 TB/s of C-tile traffic), panel solves 1.3 ms, column updates 0.95 ms, Gram 0.9 ms, diagonal blocks 0.4 ms.
// What the models do differently is handed in: prep (may be empty) runs in front of the right-hand-side rows of a chunk, gram
// builds the chunk's matrices; both launch on c->stream for sets b0 .. b0+cnt-1.
using BatchStage = std::function<void(int b0, int cnt)>;
static void batch_middle_enqueue(Ctx* c, int N, int Np, int nb, const double* ydev, const double* mean_arg, size_t mean_b, double* A,
                                 int ld, size_t bstride, double* inv16, size_t inv16_b, double* scal, int* info, const BatchStage& prep,
                                 const BatchStage& gram) {
    hipStream_t main_s = c->stream;
    static const double cache_mb = getenv("BOSS_BATCH_CHUNK_MB") ? atof(getenv("BOSS_BATCH_CHUNK_MB")) : 1e12;
    static const int max_streams = getenv("BOSS_BATCH_STREAMS") ? std::max(1, std::min(3, atoi(getenv("BOSS_BATCH_STREAMS")))) : 3;
    int cs = (int)std::min<double>((double)nb, cache_mb * 1048576.0 / ((double)bstride * sizeof(double)));
    if (cs < 12 || c->prof_on) cs = nb;                      // (large matrices, or too few per chunk for the paired batched schedule: one batch as before)
    const int nchunks = (nb + cs - 1) / cs;
    const int nstreams = std::min(max_streams, nchunks);
    if (nstreams > 1) {
        (void)hipEventRecord(c->ev_fork, main_s);
        for (int j = 1; j < nstreams; ++j) (void)hipStreamWaitEvent(c->llg_stream[j - 1], c->ev_fork, 0);
    }
    (void)hipMemsetAsync(info, 0, sizeof(int) * nb, main_s);
    if (nstreams > 1) {                                       // (the memset precedes every chunk)
        (void)hipEventRecord(c->ev_fork, main_s);
        for (int j = 1; j < nstreams; ++j) (void)hipStreamWaitEvent(c->llg_stream[j - 1], c->ev_fork, 0);
    }
    for (int ch = 0; ch < nchunks; ++ch) {
        const int b0 = (int)((long long)nb * ch / nchunks), cnt = (int)((long long)nb * (ch + 1) / nchunks) - b0;   // balanced: no small remainder chunk
        hipStream_t s = (ch % nstreams) ? c->llg_stream[ch % nstreams - 1] : main_s;
        c->stream = s;                                       // (the enqueue helpers launch on the context's current stream)
        {
            ProfScope ps(c, "prep");
            if (prep) prep(b0, cnt);
            hipLaunchKernelGGL(rhs_rows_kernel, dim3((Np + 255) / 256, 1, cnt), dim3(256), 0, s, A + (size_t)b0 * bstride, ld, bstride, N, Np,
                               ydev, mean_arg ? mean_arg + (size_t)b0 * mean_b : nullptr, mean_b, 0, (int*)nullptr);
        }
        gram(b0, cnt);
        potrf_enqueue(c, A + (size_t)b0 * bstride, ld, Np, cnt, bstride, inv16 + (size_t)b0 * inv16_b, inv16_b, info + b0, /*gates=*/false);
        {
            ProfScope ps(c, "logdet");
            hipLaunchKernelGGL(potrf_logdet_kernel, dim3(1, 1, cnt), dim3(LOGDET_THREADS), 0, s, A + (size_t)b0 * bstride, ld, bstride, N, Np,
                               scal + 2 * (size_t)b0, (double*)nullptr, (const int*)nullptr, (unsigned long long*)nullptr, 0ull, 0ull);
        }
    }
    c->stream = main_s;
    for (int j = 1; j < nstreams; ++j) {
        (void)hipEventRecord(c->llg_join[j - 1], c->llg_stream[j - 1]);
        (void)hipStreamWaitEvent(main_s, c->llg_join[j - 1], 0);
    }
}

// The plain model's stages: scaled points per set, then the stationary Gram kernel.
static void batch_factor_enqueue(Ctx* c, int kernel, int d, int N, int Np, int nb, const double* Xraw, const double* ydev,
                                 const double* mean_arg, size_t mean_b, const double* invlam, const double* hyp, double* Xsc,
                                 size_t xs_bstride, double* A, int ld, size_t bstride, double* inv16, size_t inv16_b, double* scal, int* info) {
    batch_middle_enqueue(
        c, N, Np, nb, ydev, mean_arg, mean_b, A, ld, bstride, inv16, inv16_b, scal, info,
        [&](int b0, int cnt) {
            hipLaunchKernelGGL(scale_points_kernel, dim3((Np + 255) / 256, 1, cnt), dim3(256), 0, c->stream, Xraw, Xsc + (size_t)b0 * xs_bstride,
                               xs_bstride, invlam + (size_t)b0 * d, d, Np);
        },
        [&](int b0, int cnt) {
            gram_enqueue(c, Xsc + (size_t)b0 * xs_bstride, xs_bstride, d, N, Np, kernel, hyp + 2 * (size_t)b0, A + (size_t)b0 * bstride, ld, bstride,
                         cnt);
        });
}

// What the device left of set b as the caller sees it (shared by the three models' batched likelihoods): an invalid parameter set,
// a failed pivot or a non-finite result give -Inf and their status, the others the log marginal likelihood of N observations.
static int batch_set_result(int N, bool valid, int info, double logdet, double zz, double* ll) {
    *ll = -std::numeric_limits<double>::infinity();
    if (!valid) return BOSS_E_INVALID;
    if (info != 0 || !std::isfinite(logdet) || !std::isfinite(zz)) return BOSS_E_NOT_PD;   // safe_data_loglike: exception → -Inf
    *ll = loglik(N, logdet, zz);
    return BOSS_OK;
}

// Set b of a batch — or a member of a fitted set — seen as a handle: the shape and the arrays every reader of a factor takes from
// it (block columns and leading dimension follow from the padded row count as in gp_create_common)
static void set_view(boss_gp* v, Ctx* c, int kernel, int d, int N, int Np, double* A, double* inv16, double* Xsc, double* Dinv,
                     double* Dinv2) {
    v->ctx = c;
    v->kernel = kernel;
    v->d = d;
    v->N = N;
    v->Np = Np;
    v->nblk = Np / BLK;
    v->ld = Np + RHS_ROWS;
    v->A = A;
    v->inv16 = inv16;
    v->Xsc = Xsc;
    v->Dinv = Dinv;
    v->Dinv2 = Dinv2;
}

// Padded rows up to which the gradient passes of a batch run in groups (BOSS_LLGRAD_GROUP_NP, read once per process)
static int llgrad_group_np_max() {
    static const int v = getenv("BOSS_LLGRAD_GROUP_NP") ? atoi(getenv("BOSS_LLGRAD_GROUP_NP")) : 2048;
    return v;
}
// How many sets of a chunk share one gradient pass (0: no gradients): small sets run in groups (every launch covers the group in
// grid.z, bounded by 2 GiB of work matrices), large ones set after set
static int llgrad_group_size(bool grads, int Np, int ld, int chunk) {
    if (!grads) return 0;
    const size_t per_set_w = 2 * (size_t)ld * Np * sizeof(double);
    return Np <= llgrad_group_np_max() ? (int)std::max<size_t>(1, std::min<size_t>((size_t)chunk, ((size_t)2 << 30) / per_set_w)) : 1;
}
// one set's Dinv + Dinv2, and what the gradient passes of a chunk need of them: one per bank / per member of a group
static size_t llgrad_dinv_one(int Np) { return (size_t)(Np / BLK) * BLK * BLK + (size_t)Np * PRED_RB; }
static size_t llgrad_dinv_doubles(int group, int Np) { return group ? (size_t)std::max(group, (int)Ctx::LLG_BANKS) * llgrad_dinv_one(Np) : 0; }

// set b's Jacobian and outputs from those of the chunk's first set
static MeanFold mean_fold_of_set(const MeanFold& m, int N, int b) {
    MeanFold r = m;
    if (r.J) r.J += (size_t)b * m.sJ;
    if (r.dmean) r.dmean += (size_t)b * N;
    if (r.dtheta) r.dtheta += (size_t)b * m.T;
    return r;
}

// The gradient passes of the nb factorised sets of a chunk (shared by the three models' batched likelihood gradients): in groups of
// `group` sets, or — group = 1 — set after set over up to four streams, each on its own bank of workspaces, so that their small
// kernels (low levels of the triangular inverse, reductions) overlap the other sets' large ones.  view(v, b, Dinv, Dinv2) makes v a
// view of set b as a fitted handle; St holds the constant strides between sets; set b's results go to sums + b·sum_stride and its
// α² (plain model) is read at amp2_dev[2 b].  mf (plain model, may be null): the chunk's Jacobians and the outputs of the gradient
// through the prior mean, set 0's; every set's fold runs behind its own partials of a, on that set's stream and bank.
// Everything is complete on s's timeline when the function returns.
static int llgrad_sets_enqueue(Ctx* c, hipStream_t s, int nb, int group, int Np, double* dinv_scratch, double* sums, size_t sum_stride,
                               const SetBatch& St, const double* amp2_dev,
                               const std::function<void(boss_gp*, int, double*, double*)>& view, const MeanFold* mf = nullptr) {
    const int nblk = Np / BLK;
    const size_t dinv_one = llgrad_dinv_one(Np);
    int rc = BOSS_OK;
    if (group > 1) {
        for (int b0 = 0; b0 < nb; b0 += group) {
            boss_gp v;                                       // a view of sets b0 .. b0+cnt-1 as fitted handles with constant strides
            view(&v, b0, dinv_scratch, dinv_scratch + (size_t)group * nblk * BLK * BLK);
            SetBatch B = St;
            B.nb = std::min(group, nb - b0);
            B.sDinv = (size_t)nblk * BLK * BLK;
            B.sDinv2 = (size_t)Np * PRED_RB;
            const MeanFold mb = mf ? mean_fold_of_set(*mf, v.N, b0) : MeanFold();
            rc = llgrad_enqueue(&v, s, sums + (size_t)b0 * sum_stride, 0, B, amp2_dev ? amp2_dev + 2 * (size_t)b0 : nullptr, 2, mf ? &mb : nullptr);
            if (rc) {
                (void)hipDeviceSynchronize();
                return rc;
            }
        }
        return BOSS_OK;
    }
    static const int nbanks_env = getenv("BOSS_LLGRAD_STREAMS") ? atoi(getenv("BOSS_LLGRAD_STREAMS")) : Ctx::LLG_BANKS;
    const int nbanks = std::max(1, std::min(std::min(nbanks_env, (int)Ctx::LLG_BANKS), nb));
    if (nbanks > 1) {
        (void)hipEventRecord(c->ev_fork, s);
        for (int i = 0; i < nbanks - 1; ++i) (void)hipStreamWaitEvent(c->llg_stream[i], c->ev_fork, 0);
    }
    for (int b = 0; b < nb; ++b) {                           // a view of set b as a fitted handle
        const int bank = b % nbanks;
        hipStream_t sb = bank ? c->llg_stream[bank - 1] : s;
        boss_gp v;
        double* const dinv = dinv_scratch + (size_t)bank * dinv_one;
        view(&v, b, dinv, dinv + (size_t)nblk * BLK * BLK);
        const MeanFold mb = mf ? mean_fold_of_set(*mf, v.N, b) : MeanFold();
        rc = llgrad_enqueue(&v, sb, sums + (size_t)b * sum_stride, bank, SetBatch(), amp2_dev ? amp2_dev + 2 * (size_t)b : nullptr, 0,
                            mf ? &mb : nullptr);
        if (rc) {
            (void)hipDeviceSynchronize();
            return rc;
        }
    }
    for (int i = 0; i < nbanks - 1; ++i) {
        (void)hipEventRecord(c->llg_join[i], c->llg_stream[i]);
        (void)hipStreamWaitEvent(s, c->llg_join[i], 0);
    }
    return BOSS_OK;
}

// the matrices of one chunk of a batched likelihood stay below this many bytes: 12 GiB, or BOSS_MODEL_BATCH_CHUNK_MB=<MB> (tests)
static size_t batch_chunk_bytes() {
    static const double mb = getenv("BOSS_MODEL_BATCH_CHUNK_MB") ? atof(getenv("BOSS_MODEL_BATCH_CHUNK_MB")) : 12288.0;
    return (size_t)(std::max(mb, 0.0) * 1048576.0);
}

// grad_out: null, or (d+2)×S — ∂logpdf/∂(λ_1..λ_d, α, σ) of every set (the factorisations run batched, the gradient passes set
// after set on the shared workspaces).  mean (boss_gp_loglike_grad_batch_mean, with grad_out): the Jacobians of the prior means and
// where ∂logpdf/∂mean_X (N×S) and its fold with them (T×S) go, host pointers; the Jacobians are staged per chunk as the means are,
// and the two results come back in the chunk's copy-back behind the Σ-vectors.
// BOSS_MODEL_BATCH_CHUNK_MB=<MB> (tests) lowers the 12 GiB limit as in model_loglike_batch_run below.
struct BatchMeanGrad {
    int T = 0;
    const double* jac = nullptr;
    int jac_stride = 0;
    double* dmean_out = nullptr;
    double* dtheta_out = nullptr;
};
static int loglike_batch_impl(int device, int kernel, int d, int N, const double* X, const double* y,
                              const double* mean_X, int mean_stride, const unsigned char* discrete, int S,
                              const double* lengthscales, const double* amplitudes, const double* noise_stds,
                              double* ll_out, int* status_out, double* grad_out, const BatchMeanGrad* mean = nullptr) {
    if (kernel < 0 || kernel > 2) return fail(BOSS_E_INVALID, "unknown kernel id");
    if (grad_out && d > LLG_MAX_D) return fail(BOSS_E_INVALID, "x_dim too large for the likelihood-gradient kernel");
    if (d < 1 || N < 1 || S < 0 || !X || !y || !ll_out) return fail(BOSS_E_INVALID, "bad arguments");
    if (N > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");   // 32-bit element offsets in the kernels
    if (S == 0) return BOSS_OK;
    if (!lengthscales || !amplitudes || !noise_stds) return fail(BOSS_E_INVALID, "NULL hyper-parameter array");
    if (mean_X && mean_stride != 0 && mean_stride != N) return fail(BOSS_E_INVALID, "mean_stride must be 0 or N");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const int Np = round_up(N, grad_out ? PRED_RB : BLK), nblk = Np / BLK, ld = Np + RHS_ROWS;   // the gradient pass works in 256-row steps
    const size_t bstride = (size_t)ld * Np;
    // chunk the batch so the matrices stay below ~12 GiB
    size_t per = bstride * sizeof(double);
    int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)S, batch_chunk_bytes() / per));
    const size_t xs_bstride = (size_t)d * Np;
    // the gradient through the prior mean: T columns folded on the device (0: none), per set N values of a and T of the fold
    const int T = (mean && mean->dtheta_out) ? mean->T : 0;
    const size_t jac_one = (size_t)N * T, jac_doubles = T ? (mean->jac_stride ? jac_one * chunk : jac_one) : 0;
    const size_t mg_n = (mean && mean->dmean_out) ? (size_t)N : 0, mg_doubles = mg_n + T;
    rc = ws_reserve(c->batchA, per * chunk);
    if (rc) return rc;
    rc = ws_reserve(c->batchX, sizeof(double) * (xs_bstride * (chunk + 1) + (size_t)Np * (chunk + 1) + jac_doubles));
    if (rc) return rc;
    const size_t inv16_b = (size_t)nblk * 8 * 256;
    const int nv = d + 2;
    // small sets run their gradient passes in groups (every launch covers the group in grid.z), large ones set after set
    const int group = llgrad_group_size(grad_out != nullptr, Np, ld, chunk);
    const size_t dinv_doubles = llgrad_dinv_doubles(group, Np);
    rc = ws_reserve(c->batchMisc, sizeof(double) * ((size_t)chunk * (inv16_b + 2 + 2 + d + nv + mg_doubles) + dinv_doubles) + sizeof(int) * chunk + 64);
    if (rc) return rc;
    double* A = (double*)c->batchA.p;
    double* Xraw = (double*)c->batchX.p;               // raw points | y | prior means lie together: one upload for small problems
    double* ydev = Xraw + xs_bstride;
    double* meandev = ydev + Np;                       // chunk × Np (or Np when shared)
    double* Xsc = meandev + (size_t)Np * chunk;
    double* jacdev = Xsc + xs_bstride * chunk;              // chunk × N×T (or one N×T when shared)
    double* inv16 = (double*)c->batchMisc.p;
    double* hyp = inv16 + inv16_b * chunk;
    double* scal = hyp + 2 * (size_t)chunk;
    double* invlam = scal + 2 * (size_t)chunk;
    double* sums = invlam + (size_t)d * chunk;              // chunk × (d+2) | chunk × N (a) | chunk × T (fold): one copy back
    double* dmeandev = sums + (size_t)nv * chunk;
    double* dthetadev = dmeandev + mg_n * chunk;
    double* dinv_scratch = dthetadev + (size_t)T * chunk;
    int* info = (int*)(dinv_scratch + dinv_doubles);

    std::vector<double> buf;
    pack_points(buf, X, d, N, Np, discrete);
    std::vector<double> yb(Np, 0.0);
    std::copy(y, y + N, yb.begin());
    // Small problems in one chunk (the reference's own sizes, called hundreds of times per fit): the inputs travel through the
    // pinned staging area in two asynchronous copies — [points | y | means] and [α²,σ² | (results) | 1/λ] — instead of five
    // blocking ones.  The area is free again when the call returns (it ends with a stream synchronisation).
    const size_t mean_doubles = mean_X ? (mean_stride == 0 ? (size_t)Np : (size_t)Np * S) : 0;
    const size_t up1 = xs_bstride + Np + mean_doubles, up2 = (size_t)S * (4 + d);
    const bool staged = chunk >= S && sizeof(double) * (up1 + up2) <= PINNED_UP_BYTES;
    double* stage = (double*)((char*)c->pinned + PINNED_UP_OFF);
    if (staged) {
        HIPCHK(hipEventSynchronize(c->ev_up));
        std::memcpy(stage, buf.data(), sizeof(double) * xs_bstride);
        std::memcpy(stage + xs_bstride, yb.data(), sizeof(double) * Np);
    } else {
        HIPCHK(hipMemcpy(Xraw, buf.data(), sizeof(double) * xs_bstride, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ydev, yb.data(), sizeof(double) * Np, hipMemcpyHostToDevice));
    }

    std::vector<double> h_invlam((size_t)d * chunk), h_hyp(2 * (size_t)chunk), h_scal(2 * (size_t)chunk), h_mean;
    std::vector<int> h_info(chunk), valid(chunk);
    std::vector<double> h_sums;
    MeanFold mf;                                             // (the device side of `mean`, set 0 of a chunk)
    if (mg_doubles) {
        mf.J = T ? jacdev : nullptr;
        mf.sJ = (T && mean->jac_stride) ? jac_one : 0;
        mf.T = T;
        mf.dmean = mg_n ? dmeandev : nullptr;
        mf.dtheta = T ? dthetadev : nullptr;
        if (T && !mean->jac_stride) HIPCHK(hipMemcpyAsync(jacdev, mean->jac, sizeof(double) * jac_one, hipMemcpyHostToDevice, s));
    }
    // what comes back per chunk: the Σ-vectors, then a and the fold where they are asked for, contiguous on the device
    const auto sums_back = [&](int nb) {
        h_sums.resize(((size_t)nv + mg_doubles) * chunk);
        if (!mg_doubles) return hipMemcpyAsync(h_sums.data(), sums, sizeof(double) * nv * nb, hipMemcpyDeviceToHost, s);
        return hipMemcpyAsync(h_sums.data(), sums, sizeof(double) * (((size_t)nv + mg_n) * chunk + (size_t)T * nb), hipMemcpyDeviceToHost, s);
    };
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int nb = std::min(chunk, S - s0);
        if (T && mean->jac_stride)
            HIPCHK(hipMemcpyAsync(jacdev, mean->jac + (size_t)s0 * jac_one, sizeof(double) * jac_one * nb, hipMemcpyHostToDevice, s));
        for (int b = 0; b < nb; ++b)
            valid[b] = stage_hyper(d, lengthscales + (size_t)(s0 + b) * d, amplitudes[s0 + b], noise_stds[s0 + b], &h_invlam[(size_t)b * d],
                                   &h_hyp[2 * b]);
        if (!staged) {
            HIPCHK(hipMemcpy(invlam, h_invlam.data(), sizeof(double) * d * nb, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(hyp, h_hyp.data(), sizeof(double) * 2 * nb, hipMemcpyHostToDevice));
        }
        size_t mean_b = 0;
        const double* mean_arg = nullptr;
        if (mean_X) {
            if (mean_stride == 0) {
                h_mean.assign(Np, 0.0);
                std::copy(mean_X, mean_X + N, h_mean.begin());
                if (!staged) HIPCHK(hipMemcpy(meandev, h_mean.data(), sizeof(double) * Np, hipMemcpyHostToDevice));
            } else {
                h_mean.assign((size_t)Np * nb, 0.0);
                for (int b = 0; b < nb; ++b)
                    std::copy(mean_X + (size_t)(s0 + b) * N, mean_X + (size_t)(s0 + b + 1) * N, h_mean.begin() + (size_t)b * Np);
                if (!staged) HIPCHK(hipMemcpy(meandev, h_mean.data(), sizeof(double) * Np * nb, hipMemcpyHostToDevice));
                mean_b = Np;
            }
            mean_arg = meandev;
        }
        if (staged) {
            // (one chunk: nb == S) device layout: Xraw | y | means contiguous; hyp | scal | invlam contiguous
            if (mean_X) std::memcpy(stage + xs_bstride + Np, h_mean.data(), sizeof(double) * h_mean.size());
            double* st2 = stage + up1;
            std::memcpy(st2, h_hyp.data(), sizeof(double) * 2 * nb);
            std::memcpy(st2 + 4 * (size_t)chunk, h_invlam.data(), sizeof(double) * d * nb);
            HIPCHK(hipMemcpyAsync(Xraw, stage, sizeof(double) * (xs_bstride + Np + (mean_X ? h_mean.size() : 0)), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(hyp, st2, sizeof(double) * (4 * (size_t)chunk + (size_t)d * nb), hipMemcpyHostToDevice, s));
            HIPCHK(hipEventRecord(c->ev_up, s));
        }
        if (small_fit_ok(c, N, d)) {
            // the reference's own sizes: one workgroup per set does scaled points, Gram, factorisation, z, logdet (small_fit_batch_kernel),
            // a second launch the Σ-vectors of the gradients (small_llgrad_kernel) — two launches per chunk instead of a dozen per group
            hipLaunchKernelGGL(small_fit_batch_kernel, dim3(nb), dim3(DIAG_THREADS), SMALL_LDS_BYTES, s, d, N, Np, ld, kernel,
                               (const double*)invlam, (const double*)hyp, (const double*)Xraw, Xsc, xs_bstride, (const double*)ydev,
                               mean_arg, mean_b, A, bstride, inv16, inv16_b, scal, info);
            if (grad_out) {
                hipLaunchKernelGGL(small_llgrad_kernel, dim3(nb), dim3(DIAG_THREADS), SMALL_LLG_LDS_BYTES, s, (const double*)A, ld, Np, N, d,
                                   kernel, 0.0, (const double*)inv16, (const double*)Xsc, Np, sums, bstride, inv16_b, xs_bstride,
                                   (const double*)hyp, 2, nv, 0ull, mf.J, T, mf.sJ, mf.dmean, mf.dtheta);
                HIPCHK(sums_back(nb));
            }
        } else {
        batch_factor_enqueue(c, kernel, d, N, Np, nb, Xraw, ydev, mean_arg, mean_b, invlam, hyp, Xsc, xs_bstride, A, ld, bstride, inv16, inv16_b,
                             scal, info);
        if (grad_out) {
            SetBatch St;
            St.sA = bstride;
            St.sInv16 = inv16_b;
            St.sX = xs_bstride;
            rc = llgrad_sets_enqueue(c, s, nb, group, Np, dinv_scratch, sums, nv, St, hyp, [&](boss_gp* v, int b, double* Dinv, double* Dinv2) {
                set_view(v, c, kernel, d, N, Np, A + (size_t)b * bstride, inv16 + (size_t)b * inv16_b, Xsc + (size_t)b * xs_bstride, Dinv, Dinv2);
            }, mg_doubles ? &mf : nullptr);
            if (rc) return rc;
            HIPCHK(sums_back(nb));
        }
        }   // !small
        HIPCHK(hipMemcpyAsync(h_scal.data(), scal, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_info.data(), info, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        for (int b = 0; b < nb; ++b) {
            const double logdet = h_scal[2 * b], zz = h_scal[2 * b + 1];
            double ll;
            const int st = batch_set_result(N, valid[b], h_info[b], logdet, zz, &ll);
            ll_out[s0 + b] = ll;
            if (status_out) status_out[s0 + b] = st;
            if (grad_out) {
                double* gr = grad_out + (size_t)(s0 + b) * nv;
                if (st == BOSS_OK)
                    llgrad_finalize(d, N, &h_invlam[(size_t)b * d], h_hyp[2 * b], h_hyp[2 * b + 1], zz, &h_sums[(size_t)b * nv], gr);
                else
                    for (int m = 0; m < nv; ++m) gr[m] = 0.0;
            }
            // (a set without a factor gets zeros, like its gradient)
            if (mg_n) {
                const double* a = &h_sums[(size_t)nv * chunk + (size_t)b * N];
                for (int j = 0; j < N; ++j) mean->dmean_out[(size_t)(s0 + b) * N + j] = st == BOSS_OK ? a[j] : 0.0;
            }
            if (T) {
                const double* t = &h_sums[((size_t)nv + mg_n) * chunk + (size_t)b * T];
                for (int k = 0; k < T; ++k) mean->dtheta_out[(size_t)(s0 + b) * T + k] = st == BOSS_OK ? t[k] : 0.0;
            }
        }
    }
    return BOSS_OK;
}

extern "C" int boss_gp_loglike_batch(int device, int kernel, int d, int N, const double* X, const double* y,
                                     const double* mean_X, int mean_stride, const unsigned char* discrete, int S,
                                     const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                     double* ll_out, int* status_out) {
    return loglike_batch_impl(device, kernel, d, N, X, y, mean_X, mean_stride, discrete, S, lengthscales, amplitudes, noise_stds,
                              ll_out, status_out, nullptr);
}

// S log marginal likelihoods AND their gradients w.r.t. (lengthscale[d], amplitude, noise_std): what a multistart
// OptimizationMAP evaluates per round (src/model_fitters/optimization.jl:146-164), all starts in one call.
extern "C" int boss_gp_loglike_grad_batch(int device, int kernel, int d, int N, const double* X, const double* y,
                                          const double* mean_X, int mean_stride, const unsigned char* discrete, int S,
                                          const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                          double* ll_out, double* grad_out, int* status_out) {
    if (!grad_out) return fail(BOSS_E_INVALID, "grad_out is NULL");
    return loglike_batch_impl(device, kernel, d, N, X, y, mean_X, mean_stride, discrete, S, lengthscales, amplitudes, noise_stds,
                              ll_out, status_out, grad_out);
}

// boss_gp_loglike_grad_batch plus the gradient through the prior mean: ∂logpdf/∂mean_X[j] = (K⁻¹(y − m))_j of every set (dmean_out,
// N×S) and its fold with the Jacobian of the mean values w.r.t. T parameters of a parametric mean (dtheta_out, T×S) — what
// OptimizationMAP's AD carries into θ of a Semiparametric model (src/models/semiparametric.jl:79-92).  ll_out, grad_out and
// status_out are boss_gp_loglike_grad_batch's in every bit: the same launches produce them, the fold only reads their workspace.
extern "C" int boss_gp_loglike_grad_batch_mean(int device, int kernel, int d, int N, const double* X, const double* y,
                                               const double* mean_X, int mean_stride, const unsigned char* discrete, int S,
                                               const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                               int T, const double* mean_jac, int jac_stride, double* ll_out, double* grad_out,
                                               double* dmean_out, double* dtheta_out, int* status_out) {
    if (!grad_out) return fail(BOSS_E_INVALID, "grad_out is NULL");
    if (T < 0) return fail(BOSS_E_INVALID, "T must be >= 0");
    if (T > 0 && !mean_jac) return fail(BOSS_E_INVALID, "mean_jac is NULL");
    if (T == 0 && dtheta_out) return fail(BOSS_E_INVALID, "dtheta_out needs T > 0");
    if (jac_stride != 0 && (long long)jac_stride != (long long)N * T)
        return fail(BOSS_E_INVALID, "jac_stride must be 0 or N*T");
    BatchMeanGrad mg;
    mg.T = mean_jac ? T : 0;
    mg.jac = mean_jac;
    mg.jac_stride = jac_stride;
    mg.dmean_out = dmean_out;
    mg.dtheta_out = dtheta_out;
    return loglike_batch_impl(device, kernel, d, N, X, y, mean_X, mean_stride, discrete, S, lengthscales, amplitudes, noise_stds,
                              ll_out, status_out, grad_out, &mg);
}

// ------------------------------------------------------------------------------------------
// Batched likelihoods of the gradient-observation and the nonstationary model (boss_ggp_loglike_batch, boss_ngp_loglike_batch):
// `loglike.(samples)` of src/model_fitters/sampling.jl:59-78 over gradient_gp.jl:367-397 / nonstationary_gp.jl:237-245.  The
// structure is loglike_batch_impl's: chunks of at most 12 GiB of matrices on the workspaces batchA / batchX / batchMisc, the shared
// middle (batch_middle_enqueue), one copy back and one synchronisation per chunk.  The models differ in their resident points, in
// the per-set parameter block (par_doubles doubles per set, written by fill, which also says whether the set is valid) and in the
// Gram launch.  Rows are padded to 128 (the one-workgroup small path knows the plain kernel only).
// BOSS_MODEL_BATCH_CHUNK_MB=<MB> (tests) lowers the 12 GiB limit so that a small batch spans several chunks.
// With gradients (boss_ggp_loglike_grad_batch, boss_ngp_loglike_grad_batch; ModelBatchGrad) the caller pads the rows to 256, since
// the gradient pass works in 256-row steps — the extra identity block changes no sum, the likelihoods stay those of the 128-padded
// call in every bit —, and the gradient passes of a chunk follow its factorisations under the plain model's grouping policy
// (llgrad_sets_enqueue); their results come back in the chunk's one copy and one synchronisation.
// ------------------------------------------------------------------------------------------
struct ModelBatchGramArgs {
    const double* pts;                                       // the model's points, shared by all sets
    const double* par;                                       // first set of the chunk, par_doubles apart
    double* A;
    int ld, cnt;
    size_t bstride;
};
struct ModelBatchGrad {
    size_t out_doubles;                                      // results per set on the device: d+3 sums, or (d+3)·Np per-point values
    std::function<void(boss_gp*, const double* pts_dev, double* par_dev)> view;   // what llgrad_enqueue reads of the model in a view of one set
    std::function<void(int s, const double* par, const double* h)> finish;       // set s's outputs from its staged parameters and results; h null: zeros
};

// Two optional hooks make a whole-chain call of it (boss_nfit_loglike_grad, host_nfit.inc): the parameter blocks of a chunk are
// written ON THE DEVICE (`fill` enqueues that on c->stream and raises flags[b] != 0 for an invalid set; the flags come back with the
// failed-pivot flags in one copy), and the gradient pass's results are consumed on the device (`consume` enqueues kernels and its
// own copy back behind them; `finish` runs after the chunk's synchronisation).  The host `fill` and G->finish are not called then.
struct ModelBatchDevice {
    std::function<int(int s0, int nb, double* par_dev, int* flags_dev)> fill;
    std::function<int(int s0, int nb, const double* sums_dev)> consume;      // null: nothing to consume (likelihoods only)
    std::function<void(int s, int b, int status)> finish;                    // set s = member b of the chunk just synchronised
};

static int model_loglike_batch_run(Ctx* c, int N, int Np, int S, const std::vector<double>& pts, const std::vector<double>& yb,
                                   const double* mean_X, int mean_stride, size_t par_doubles,
                                   const std::function<bool(int, double*)>& fill,
                                   const std::function<void(const ModelBatchGramArgs&)>& gram, double* ll_out, int* status_out,
                                   const ModelBatchGrad* G = nullptr, const ModelBatchDevice* Dv = nullptr) {
    hipStream_t s = c->stream;
    const int nblk = Np / BLK, ld = Np + RHS_ROWS;
    const size_t bstride = (size_t)ld * Np, per = bstride * sizeof(double);
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)S, batch_chunk_bytes() / per));
    const size_t inv16_b = (size_t)nblk * 8 * 256, mean_doubles = mean_X ? (mean_stride == 0 ? (size_t)Np : (size_t)Np * chunk) : 0;
    int rc = ws_reserve(c->batchA, per * chunk);
    if (rc) return rc;
    rc = ws_reserve(c->batchX, sizeof(double) * (pts.size() + Np + mean_doubles + par_doubles * chunk));
    if (rc) return rc;
    const int group = llgrad_group_size(G != nullptr, Np, ld, chunk);
    const size_t dinv_doubles = llgrad_dinv_doubles(group, Np), out_doubles = G ? G->out_doubles : 0;
    rc = ws_reserve(c->batchMisc, sizeof(double) * ((size_t)chunk * (inv16_b + 2 + out_doubles) + dinv_doubles) + sizeof(int) * chunk * (Dv ? 2 : 1) + 64);
    if (rc) return rc;
    double* A = (double*)c->batchA.p;
    double* pts_dev = (double*)c->batchX.p;                  // points | observations | prior means | parameter blocks
    double* ydev = pts_dev + pts.size();
    double* meandev = ydev + Np;
    double* par_dev = meandev + mean_doubles;
    double* inv16 = (double*)c->batchMisc.p;
    double* scal = inv16 + inv16_b * chunk;
    double* sums = scal + 2 * (size_t)chunk;                 // chunk × out_doubles
    double* dinv_scratch = sums + out_doubles * chunk;
    int* info = (int*)(dinv_scratch + dinv_doubles);
    std::vector<double> h_sums(Dv ? 0 : out_doubles * chunk);
    // (the host vectors outlive the copies: every chunk ends with a synchronisation)
    HIPCHK(hipMemcpyAsync(pts_dev, pts.data(), sizeof(double) * pts.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ydev, yb.data(), sizeof(double) * Np, hipMemcpyHostToDevice, s));
    std::vector<double> h_par(Dv ? 0 : par_doubles * chunk), h_scal(2 * (size_t)chunk), h_mean;
    std::vector<int> h_info(chunk * (Dv ? 2 : 1)), valid(chunk);   // (device fill: failed-pivot flags | validity flags)
    const int Nm = mean_X ? mean_stride : 0;                 // (mean_stride is 0 or the number of observations)
    if (mean_X && mean_stride == 0) {
        h_mean.assign(Np, 0.0);
        std::copy(mean_X, mean_X + N, h_mean.begin());
        HIPCHK(hipMemcpyAsync(meandev, h_mean.data(), sizeof(double) * Np, hipMemcpyHostToDevice, s));
    }
    for (int s0 = 0; s0 < S; s0 += chunk) {
        const int nb = std::min(chunk, S - s0);
        if (Dv) {
            HIPCHK(hipMemsetAsync(info + nb, 0, sizeof(int) * nb, s));
            if ((rc = Dv->fill(s0, nb, par_dev, info + nb)) != BOSS_OK) {
                (void)hipStreamSynchronize(s);
                return rc;
            }
        } else {
            for (int b = 0; b < nb; ++b) valid[b] = fill(s0 + b, h_par.data() + (size_t)b * par_doubles);
            HIPCHK(hipMemcpyAsync(par_dev, h_par.data(), sizeof(double) * par_doubles * nb, hipMemcpyHostToDevice, s));
        }
        if (Nm) {
            h_mean.assign((size_t)Np * nb, 0.0);
            for (int b = 0; b < nb; ++b)
                std::copy(mean_X + (size_t)(s0 + b) * Nm, mean_X + (size_t)(s0 + b + 1) * Nm, h_mean.begin() + (size_t)b * Np);
            HIPCHK(hipMemcpyAsync(meandev, h_mean.data(), sizeof(double) * Np * nb, hipMemcpyHostToDevice, s));
        }
        batch_middle_enqueue(c, N, Np, nb, ydev, mean_X ? meandev : nullptr, Nm ? (size_t)Np : 0, A, ld, bstride, inv16, inv16_b, scal, info,
                             BatchStage(), [&](int b0, int cnt) {
                                 ProfScope ps(c, "gram");
                                 gram(ModelBatchGramArgs{pts_dev, par_dev + (size_t)b0 * par_doubles, A + (size_t)b0 * bstride, ld, cnt, bstride});
                             });
        if (G) {
            SetBatch St;
            St.sA = bstride;
            St.sInv16 = inv16_b;
            St.sPar = par_doubles;
            rc = llgrad_sets_enqueue(c, s, nb, group, Np, dinv_scratch, sums, out_doubles, St, nullptr,
                                     [&](boss_gp* v, int b, double* Dinv, double* Dinv2) {
                                         set_view(v, c, 0, 0, N, Np, A + (size_t)b * bstride, inv16 + (size_t)b * inv16_b, nullptr, Dinv, Dinv2);
                                         G->view(v, pts_dev, par_dev + (size_t)b * par_doubles);
                                     });
            if (rc) return rc;
            if (!Dv) HIPCHK(hipMemcpyAsync(h_sums.data(), sums, sizeof(double) * out_doubles * nb, hipMemcpyDeviceToHost, s));
            else if (Dv->consume && (rc = Dv->consume(s0, nb, sums)) != BOSS_OK) {
                (void)hipStreamSynchronize(s);
                return rc;
            }
        }
        HIPCHK(hipMemcpyAsync(h_scal.data(), scal, sizeof(double) * 2 * nb, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_info.data(), info, sizeof(int) * nb * (Dv ? 2 : 1), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
        for (int b = 0; b < nb; ++b) {
            if (Dv) valid[b] = h_info[nb + b] == 0;
            const int st = batch_set_result(N, valid[b], h_info[b], h_scal[2 * b], h_scal[2 * b + 1], &ll_out[s0 + b]);
            if (status_out) status_out[s0 + b] = st;
            if (Dv) {
                if (Dv->finish) Dv->finish(s0 + b, b, st);
                continue;
            }
            if (G) G->finish(s0 + b, h_par.data() + (size_t)b * par_doubles, st == BOSS_OK ? h_sums.data() + (size_t)b * out_doubles : nullptr);
        }
    }
    return BOSS_OK;
}

// The parameter block of set b of a GradientGaussianProcess batch as a handle keeps it: 1/λ (d) | α², σ², σ_∂², - ; every
// parameter gets +1e-8 (gradient_gp.jl:128-131, :200-204) as in boss_ggp_update.  False: an invalid set, staged as all-ones.
static bool ggp_stage_set(int d, const double* lam, double amp, double sig, double gsig, double* p) {
    const bool ok = stage_hyper(d, lam, amp, sig, p, p + d) && gsig >= 0.0;
    const double sgd = (ok ? gsig : 1.0) + MIN_PARAM_VALUE;
    p[d + 2] = sgd * sgd;
    p[d + 3] = 0.0;
    return ok;
}
// ... and of a NonstationaryGP batch: λ [d][Np] | α [Np] | σ [Np], padding λ = 1, α = σ = 0 as in boss_ngp_update; the values are
// taken as given and checked as boss_ngp_update checks them.
static bool ngp_stage_set(int d, int N, int Np, const double* lam, const double* amp, const double* noi, double* p) {
    bool ok = true;
    for (int j = 0; j < N && ok; ++j) {
        for (int k = 0; k < d; ++k) ok = ok && lam[(size_t)j * d + k] > 0.0 && std::isfinite(lam[(size_t)j * d + k]);
        ok = ok && amp[j] >= 0.0 && std::isfinite(amp[j]) && noi[j] >= 0.0 && std::isfinite(noi[j]);
    }
    std::fill(p, p + (size_t)d * Np, 1.0);
    std::fill(p + (size_t)d * Np, p + ((size_t)d + 2) * Np, 0.0);
    for (int j = 0; j < N; ++j) {
        for (int k = 0; k < d; ++k) p[(size_t)k * Np + j] = ok ? lam[(size_t)j * d + k] : 1.0;
        p[(size_t)d * Np + j] = ok ? amp[j] : 1.0;
        p[(size_t)(d + 1) * Np + j] = ok ? noi[j] : 1.0;
    }
    return ok;
}

// S parameter sets (λ[d], α, σ, σ_∂) of a GradientGaussianProcess on one output slice; X d×n, dY d×n column-major as in
// boss_ggp_create, lengthscales d×S.  Every parameter gets +1e-8 (gradient_gp.jl:128-131, :200-204) as in boss_ggp_update.
// grad_out: null, or (d+3)×S — ∂ℓ/∂(λ_1..λ_d, α, σ, σ_∂) of every set.
static int ggp_loglike_batch_impl(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY, int S,
                                  const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                  const double* grad_noise_stds, double* ll_out, int* status_out, double* grad_out) {
    if (kernel < 0 || kernel > 2) return fail(BOSS_E_INVALID, "unknown kernel id");
    if (d < 1 || n < 1 || S < 0 || !X || !y || !dY || !ll_out) return fail(BOSS_E_INVALID, "bad arguments");
    if (d > AUG_MAX_D) return fail(BOSS_E_INVALID, "gradient observations: x_dim above 16 is not supported");
    if ((long long)n * (1 + d) > MAX_ROWS) return fail(BOSS_E_INVALID, "augmented system too large (n (1 + d) > 46080)");
    if (S == 0) return BOSS_OK;
    if (!lengthscales || !amplitudes || !noise_stds || !grad_noise_stds) return fail(BOSS_E_INVALID, "NULL hyper-parameter array");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mtx);
    const int N = n * (1 + d), Np = round_up(N, grad_out ? PRED_RB : BLK), ldx = round_up(n, 64);
    std::vector<double> pts, yb(Np, 0.0);
    pack_points(pts, X, d, n, ldx, nullptr);
    for (int j = 0; j < n; ++j) {                            // `_build_obs_vector` (gradient_gp.jl:288-302), built once for all sets
        yb[j] = y[j];
        for (int l = 0; l < d; ++l) yb[(size_t)n * (1 + l) + j] = dY[(size_t)j * d + l];
    }
    const size_t par_doubles = (size_t)d + 4;               // 1/λ (d) | α², σ², σ_∂², -: the layout of a handle's resident parameters
    auto fill = [&](int b, double* p) {
        return ggp_stage_set(d, lengthscales + (size_t)b * d, amplitudes[b], noise_stds[b], grad_noise_stds[b], p);
    };
    auto gram = [&](const ModelBatchGramArgs& a) {
        const long long t64 = Np / 64;
        hipLaunchKernelGGL(aug_gram_kernel, dim3((unsigned)(t64 * (t64 + 1) / 2), 1, a.cnt), dim3(256), 0, c->stream, a.pts, ldx, d, n, N, Np,
                           kernel, a.par + d, a.par, par_doubles, a.A, a.ld, a.bstride, 0);
    };
    ModelBatchGrad G;
    G.out_doubles = (size_t)d + 3;
    G.view = [&](boss_gp* v, const double* pts_dev, double* par) {
        v->kernel = kernel;
        v->d = d;
        v->aug = true;
        v->npts = n;
        v->nhead = n;
        v->ldx = ldx;
        v->Xraw = const_cast<double*>(pts_dev);
        v->invlam = par;
        v->hyp = par + d;
    };
    G.finish = [&](int b, const double* par, const double* h) {
        double* gr = grad_out + (size_t)b * (d + 3);
        if (h) ggp_llgrad_finalize(d, par, h, gr);
        else std::fill(gr, gr + d + 3, 0.0);
    };
    return model_loglike_batch_run(c, N, Np, S, pts, yb, nullptr, 0, par_doubles, fill, gram, ll_out, status_out, grad_out ? &G : nullptr);
}

extern "C" int boss_ggp_loglike_batch(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY, int S,
                                      const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                      const double* grad_noise_stds, double* ll_out, int* status_out) {
    return ggp_loglike_batch_impl(device, kernel, d, n, X, y, dY, S, lengthscales, amplitudes, noise_stds, grad_noise_stds, ll_out, status_out,
                                  nullptr);
}

// ... AND their gradients w.r.t. (lengthscale[d], amplitude, noise_std, grad_noise_std): what a multistart OptimizationMAP over a
// GradientGaussianProcess evaluates per round (src/model_fitters/optimization.jl:146-164 over gradient_gp.jl:367-397), all starts in
// one call.  Column s of grad_out is what boss_ggp_loglike_grad returns after boss_ggp_update at the parameters of set s.
extern "C" int boss_ggp_loglike_grad_batch(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY,
                                           int S, const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                           const double* grad_noise_stds, double* ll_out, double* grad_out, int* status_out) {
    if (!grad_out) return fail(BOSS_E_INVALID, "grad_out is NULL");
    return ggp_loglike_batch_impl(device, kernel, d, n, X, y, dY, S, lengthscales, amplitudes, noise_stds, grad_noise_stds, ll_out, status_out,
                                  grad_out);
}

// What the two nonstationary callers of model_loglike_batch_run (ngp_loglike_batch_impl; boss_nfit_loglike_grad, host_nfit.inc) share:
// the Gram launch over parameter blocks λ [d][Np] | α [Np] | σ [Np] and the view of one set the gradient pass reads.  One copy, so
// that the whole-chain call stays bit for bit the array call.
static void ngp_batch_gram(Ctx* c, int d, int N, int Np, const ModelBatchGramArgs& a) {
    const size_t par_doubles = ((size_t)d + 2) * Np;
    const int t64 = Np / 64;
    hipLaunchKernelGGL(gibbs_gram_kernel, dim3(t64 * (t64 + 1) / 2, 1, a.cnt), dim3(256), 0, c->stream, a.pts, a.par,
                       a.par + (size_t)d * Np, a.par + (size_t)(d + 1) * Np, par_doubles, par_doubles, d, N, Np, a.A, a.ld, a.bstride, 0);
}
static void ngp_batch_view(boss_gp* v, int d, int Np, const double* pts_dev, double* par) {
    v->d = d;
    v->gibbs = true;
    v->Xraw = const_cast<double*>(pts_dev);
    v->lamX = par;
    v->ampX = par + (size_t)d * Np;
    v->noiseX = par + (size_t)(d + 1) * Np;
}

// S sets of latent values (λ(x_j) d×N, α(x_j) N, σ(x_j) N; set after set) of a NonstationaryGP on one output slice.  The values
// are taken as given (nothing is added), and checked as boss_ngp_update checks them: a set with a lengthscale that is not finite
// and positive, or an amplitude or noise that is not finite and non-negative, is reported and the others are computed.
// grads: the partial derivatives w.r.t. the latent values are wanted (each of the four outputs may still be null).
static int ngp_loglike_batch_impl(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete, int S,
                                  const double* lam_X, const double* amp_X, const double* noise_X, const double* mean_X, int mean_stride,
                                  double* ll_out, int* status_out, bool grads, double* dlam_out, double* damp_out, double* dnoise_out,
                                  double* dmean_out) {
    if (d < 1 || N < 1 || S < 0 || !X || !y || !ll_out) return fail(BOSS_E_INVALID, "bad arguments");
    if (N > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");
    if (grads && d > GIBBS_GRAD_MAX_D) return fail(BOSS_E_INVALID, "x_dim above 16 is not supported by the nonstationary gradient kernels");
    if (S == 0) return BOSS_OK;
    if (!lam_X || !amp_X || !noise_X) return fail(BOSS_E_INVALID, "NULL latent-value array");
    if (mean_X && mean_stride != 0 && mean_stride != N) return fail(BOSS_E_INVALID, "mean_stride must be 0 or N");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mtx);
    const int Np = round_up(N, grads ? PRED_RB : BLK);
    std::vector<double> pts, yb(Np, 0.0);
    pack_points(pts, X, d, N, Np, discrete);
    std::copy(y, y + N, yb.begin());
    const size_t par_doubles = ((size_t)d + 2) * Np;        // λ [d][Np] | α [Np] | σ [Np]; padding λ = 1, α = σ = 0 as in boss_ngp_update
    auto fill = [&](int b, double* p) {
        return ngp_stage_set(d, N, Np, lam_X + (size_t)b * d * N, amp_X + (size_t)b * N, noise_X + (size_t)b * N, p);
    };
    auto gram = [&](const ModelBatchGramArgs& a) { ngp_batch_gram(c, d, N, Np, a); };
    ModelBatchGrad G;
    G.out_doubles = ((size_t)d + 3) * Np;                    // dlam [d][Np] | damp [Np] | dnoise [Np] | dmean [Np]
    G.view = [&](boss_gp* v, const double* pts_dev, double* par) { ngp_batch_view(v, d, Np, pts_dev, par); };
    G.finish = [&](int b, const double*, const double* h) {
        double* dl = dlam_out ? dlam_out + (size_t)b * d * N : nullptr;
        for (int j = 0; j < N; ++j) {
            if (dl)
                for (int k = 0; k < d; ++k) dl[(size_t)j * d + k] = h ? h[(size_t)k * Np + j] : 0.0;
            if (damp_out) damp_out[(size_t)b * N + j] = h ? h[(size_t)d * Np + j] : 0.0;
            if (dnoise_out) dnoise_out[(size_t)b * N + j] = h ? h[(size_t)(d + 1) * Np + j] : 0.0;
            if (dmean_out) dmean_out[(size_t)b * N + j] = h ? h[(size_t)(d + 2) * Np + j] : 0.0;
        }
    };
    return model_loglike_batch_run(c, N, Np, S, pts, yb, mean_X, mean_stride, par_doubles, fill, gram, ll_out, status_out, grads ? &G : nullptr);
}

extern "C" int boss_ngp_loglike_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete, int S,
                                      const double* lam_X, const double* amp_X, const double* noise_X, const double* mean_X,
                                      int mean_stride, double* ll_out, int* status_out) {
    return ngp_loglike_batch_impl(device, d, N, X, y, discrete, S, lam_X, amp_X, noise_X, mean_X, mean_stride, ll_out, status_out, false,
                                  nullptr, nullptr, nullptr, nullptr);
}

// ... AND their partial derivatives w.r.t. the latent models' values at the training points (boss_ngp_loglike_grad per set):
// dlam_out d×N×S (set after set, each in lam_X's layout), damp_out, dnoise_out, dmean_out N×S; each may be NULL.
extern "C" int boss_ngp_loglike_grad_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                                           int S, const double* lam_X, const double* amp_X, const double* noise_X,
                                           const double* mean_X, int mean_stride, double* ll_out, double* dlam_out, double* damp_out,
                                           double* dnoise_out, double* dmean_out, int* status_out) {
    return ngp_loglike_batch_impl(device, d, N, X, y, discrete, S, lam_X, amp_X, noise_X, mean_X, mean_stride, ll_out, status_out, true,
                                  dlam_out, damp_out, dnoise_out, dmean_out);
}

// ------------------------------------------------------------------------------------------
// boss_gp_fit_batch: S RESIDENT posteriors of one output slice out of ONE batched factorisation — the posteriors of the S
// hyper-parameter samples of a Bayesian-inference fit (src/posterior.jl:15-19 builds one per sample; the samples come from
// ext/TuringExt.jl:88-107 or any sampler).  X and y are uploaded once and shared by all members; Gram matrices, factors, z,
// log-likelihoods and the diagonal-block inverses the prediction kernels need are built for all sets in the same launches
// (grid.z = set), into one slab whose per-set strides are constant.  The members are ordinary handles (views into the slab).
// ------------------------------------------------------------------------------------------
__global__ void set_scatter_kernel(int d, int S, const double* __restrict__ invlamB, const double* __restrict__ hypB,
                                   const double* __restrict__ scalB, const int* __restrict__ infoB, double* __restrict__ par,
                                   size_t sPar, double* __restrict__ scal, size_t sScal) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S) return;
    if (invlamB) {                                           // (null: the members' parameter blocks were uploaded in place)
        double* p = par + (size_t)b * sPar;                  // [1/λ (d) | α², σ², -, -]: the layout of a handle's resident hyper-parameters
        for (int k = 0; k < d; ++k) p[k] = invlamB[(size_t)b * d + k];
        p[d] = hypB[2 * b];
        p[d + 1] = hypB[2 * b + 1];
    }
    double* q = scal + (size_t)b * sScal;                    // [logdet, zᵀz | info]
    q[0] = scalB[2 * b];
    q[1] = scalB[2 * b + 1];
    reinterpret_cast<int*>(q + 2)[0] = infoB[b];
}

// What the three fit-batch entry points share (fit_batch_run): the slab out of the context's cache or fresh, its layout, the upload of
// the shared points / observations / prior means, one synchronisation, the members as views, and the clean-up when anything fails.
// A model describes itself by its shape (FitBatchSpec) and two hooks: `factor` uploads the parameters and enqueues Gram matrices,
// factorisations and log-determinants of all sets on c->stream (scalB: {logdet, zᵀz} per set, infoB: failed-pivot flags), `member`
// fills in what only the model knows of member b (host_par, amp2) and says whether its parameters were valid.
struct FitBatchSpec {
    int kernel = 0, d = 0, N = 0, npts = 0, ldx = 0, S = 0;  // N rows per member; npts points [d][ldx] shared by all
    bool aug = false, gibbs = false, zero_slab = false;      // zero_slab: the one-workgroup kernels read what they do not write as zero
    const std::vector<double>* pts = nullptr;                // packed points, d·ldx doubles
    const std::vector<double>* yb = nullptr;                 // observations, padded to Np
    const double* mean_X = nullptr;
    int mean_stride = 0;
    const unsigned char* discrete = nullptr;
    size_t sExtra = 0;                                       // per-member doubles behind the common arrays (nonstationary: λ(X) | α(X) | σ(X))
    size_t compact_extra = 0;                                // staging of the batch kernels behind the members (plain model: 1/λ, {α², σ²} of all sets)
};
struct FitBatchSlab {
    int Np = 0, ld = 0;
    size_t total = 0, sA = 0, sInv = 0, sDinv = 0, sDinv2 = 0, sX = 0, sMean = 0, sPar = 0, sScal = 0, sExtra = 0;
    double *base = nullptr, *pts = nullptr, *y = nullptr, *A = nullptr, *inv16 = nullptr, *Dinv = nullptr, *Dinv2 = nullptr, *Xsc = nullptr,
           *mean = nullptr, *par = nullptr, *scal = nullptr, *extra = nullptr, *scalB = nullptr, *cextra = nullptr;
    int* infoB = nullptr;
    const double *scatter_invlam = nullptr, *scatter_hyp = nullptr;   // set by `factor` when the parameter blocks are scattered from compact arrays
};
static int fit_batch_run(Ctx* c, const FitBatchSpec& sp, const std::function<hipError_t(FitBatchSlab&, hipStream_t)>& factor,
                         const std::function<bool(int, boss_gp*)>& member, boss_gp_t** out, double* logpdf_out, int* status_out) {
    const int S = sp.S, d = sp.d, N = sp.N;
    FitBatchSlab L;
    const int Np = L.Np = round_up(N, PRED_RB), nblk = Np / BLK;
    L.ld = Np + RHS_ROWS;
    L.sA = (size_t)L.ld * Np;
    L.sInv = (size_t)nblk * 8 * 256;
    L.sDinv = (size_t)nblk * BLK * BLK;
    L.sDinv2 = (size_t)Np * PRED_RB;
    L.sX = (size_t)d * sp.ldx;
    L.sMean = (size_t)Np;
    L.sPar = (size_t)round_up(d + 4, 8);
    L.sScal = 8;
    L.sExtra = sp.sExtra;
    const size_t shared = L.sX + Np;                         // raw points | y
    const size_t compact = 2 * (size_t)S + (size_t)round_up(S, 2) / 2 + 8 + sp.compact_extra;   // {logdet, zᵀz}, info of the batch kernels
    const size_t total = L.total = shared + (size_t)S * (L.sA + L.sInv + L.sDinv + L.sDinv2 + L.sX + L.sMean + L.sPar + L.sScal + L.sExtra) + compact;
    const size_t hstride = 64 + L.sPar;                      // pinned doubles per member: host_res (512 bytes) | host_par
    HIPCHK(hipSetDevice(c->device));                         // (before anything is allocated: this early return leaves nothing behind)
    boss_gpset* st = new boss_gpset();
    st->ctx = c;
    std::vector<boss_gp*> hs;
    auto bail = [&](int code, const std::string& msg) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        for (boss_gp* g : hs) {
            if (g->par_ev) (void)hipEventDestroy(g->par_ev);
            if (g->dinv_ev) (void)hipEventDestroy(g->dinv_ev);
            if (g->discrete_dev) (void)hipFree(g->discrete_dev);
            delete g->kp;                                    // (program-kernel members: their copy of the program)
            delete g;
        }
        gpset_release_storage(st);
        delete st;
        for (int b = 0; b < S; ++b) out[b] = nullptr;
        return fail(code, msg);
    };
    std::unique_lock<std::mutex> lk(c->mtx);
    {
        // storage: the context's cached block of a released set if it is large enough, else fresh
        const size_t need = sizeof(double) * total, hneed = sizeof(double) * hstride * S;
        {
            std::lock_guard<std::mutex> sl(c->slab_mtx);
            if (c->slab_cache && c->slab_cache_bytes >= need) {
                st->slab = c->slab_cache;
                st->slab_bytes = c->slab_cache_bytes;
                c->slab_cache = nullptr;
                c->slab_cache_bytes = 0;
            }
            if (c->hostblk_cache && c->hostblk_cache_bytes >= hneed) {
                st->host_block = c->hostblk_cache;
                st->host_bytes = c->hostblk_cache_bytes;
                c->hostblk_cache = nullptr;
                c->hostblk_cache_bytes = 0;
            }
        }
        if (!st->slab) {
            if (dev_malloc(&st->slab, need) != hipSuccess) {   // (dev_malloc itself gives a smaller cached block back and tries once more)
                st->slab = nullptr;
                return bail(BOSS_E_ALLOC, "device allocation failed (the batch of posteriors does not fit)");
            }
            st->slab_bytes = need;
        }
        if (!st->host_block) {
            if (hipHostMalloc(&st->host_block, hneed, hipHostMallocDefault) != hipSuccess) {
                st->host_block = nullptr;
                return bail(BOSS_E_ALLOC, "pinned allocation failed");
            }
            st->host_bytes = hneed;
        }
    }
    std::memset(st->host_block, 0, sizeof(double) * hstride * S);
    double* host_dev = nullptr;
    if (hipHostGetDevicePointer((void**)&host_dev, st->host_block, 0) != hipSuccess) return bail(BOSS_E_ALLOC, "pinned allocation failed");
    hipStream_t s = c->stream;
    L.base = (double*)st->slab;
    L.pts = L.base;
    L.y = L.pts + L.sX;
    L.A = L.y + Np;
    L.inv16 = L.A + (size_t)S * L.sA;
    L.Dinv = L.inv16 + (size_t)S * L.sInv;
    L.Dinv2 = L.Dinv + (size_t)S * L.sDinv;
    L.Xsc = L.Dinv2 + (size_t)S * L.sDinv2;
    L.mean = L.Xsc + (size_t)S * L.sX;
    L.par = L.mean + (size_t)S * L.sMean;
    L.scal = L.par + (size_t)S * L.sPar;
    L.extra = L.scal + (size_t)S * L.sScal;
    L.scalB = L.extra + (size_t)S * L.sExtra;
    L.infoB = (int*)(L.scalB + 2 * (size_t)S);
    L.cextra = L.scalB + 2 * (size_t)S + (size_t)round_up(S, 2) / 2 + 8;

    std::vector<double> h_mean;
    hipError_t e = hipSuccess;
    // small problems (one identity-padded block row beyond the data): everything the kernels do not write reads as zero
    if (sp.zero_slab) e = hipMemsetAsync(st->slab, 0, sizeof(double) * total, s);
    else e = hipMemsetAsync(L.mean, 0, sizeof(double) * L.sMean * S, s);
    if (e == hipSuccess) e = hipMemcpyAsync(L.pts, sp.pts->data(), sizeof(double) * L.sX, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(L.y, sp.yb->data(), sizeof(double) * Np, hipMemcpyHostToDevice, s);
    if (sp.mean_X && e == hipSuccess) {
        h_mean.assign(L.sMean * S, 0.0);
        for (int b = 0; b < S; ++b) {
            const double* src = sp.mean_X + (sp.mean_stride == 0 ? 0 : (size_t)b * N);
            std::copy(src, src + N, h_mean.begin() + (size_t)b * Np);
        }
        e = hipMemcpyAsync(L.mean, h_mean.data(), sizeof(double) * L.sMean * S, hipMemcpyHostToDevice, s);
    }
    if (e != hipSuccess) return bail(BOSS_E_NO_DEVICE, std::string("uploading the observations: ") + hipGetErrorString(e));
    e = factor(L, s);
    if (e != hipSuccess) return bail(BOSS_E_NO_DEVICE, std::string("uploading the hyper-parameters: ") + hipGetErrorString(e));
    // (the block inverses the prediction kernels need are built for all members in one set of launches by the first prediction over
    // the set — predict_set_enqueue —, or member by member where a single member is used: a fit whose caller only wants the
    // likelihoods, or a few members, does not pay the 2.9 ms they cost at 512 × N = 1024)
    hipLaunchKernelGGL(set_scatter_kernel, dim3((S + 255) / 256), dim3(256), 0, s, d, S, L.scatter_invlam, L.scatter_hyp,
                       (const double*)L.scalB, (const int*)L.infoB, L.par, L.sPar, L.scal, L.sScal);
    std::vector<double> h_scal(2 * (size_t)S);
    std::vector<int> h_info(S);
    e = hipMemcpyAsync(h_scal.data(), L.scalB, sizeof(double) * 2 * S, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h_info.data(), L.infoB, sizeof(int) * S, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return bail(BOSS_E_NO_DEVICE, std::string("batched factorisation: ") + hipGetErrorString(e));
    bool any_disc = false;
    if (sp.discrete)
        for (int k = 0; k < d; ++k) any_disc |= sp.discrete[k] != 0;
    for (int b = 0; b < S; ++b) {
        boss_gp* g = new boss_gp();
        hs.push_back(g);
        set_view(g, c, sp.kernel, d, N, Np, L.A + (size_t)b * L.sA, L.inv16 + (size_t)b * L.sInv, L.Xsc + (size_t)b * L.sX,
                 L.Dinv + (size_t)b * L.sDinv, L.Dinv2 + (size_t)b * L.sDinv2);
        g->set = st;
        g->aug = sp.aug;
        g->gibbs = sp.gibbs;
        g->npts = sp.npts;
        g->nhead = sp.npts;
        g->ldx = sp.ldx;
        g->Xraw = L.pts;
        g->y = L.y;
        g->mean = L.mean + (size_t)b * L.sMean;
        g->invlam = L.par + (size_t)b * L.sPar;
        g->hyp = g->invlam + d;
        g->scal = L.scal + (size_t)b * L.sScal;
        g->info = (int*)(g->scal + 2);
        if (sp.gibbs) {
            g->lamX = L.extra + (size_t)b * L.sExtra;
            g->ampX = g->lamX + (size_t)d * Np;
            g->noiseX = g->ampX + Np;
        }
        g->host_res = (double*)st->host_block + (size_t)b * hstride;
        g->host_res_dev = host_dev + (size_t)b * hstride;
        g->host_par = g->host_res + 64;
        g->has_mean = sp.mean_X != nullptr;
        // (its two events are created by the member's first update — gp_update_enqueue —: 1024 event creations per 512-member fit
        // were a good part of what the call cost beyond its batched factorisation)
        if (any_disc) {
            g->discrete.assign(sp.discrete, sp.discrete + d);
            if (dev_malloc((void**)&g->discrete_dev, d) != hipSuccess) return bail(BOSS_E_ALLOC, "device allocation failed");
            (void)hipMemcpy(g->discrete_dev, sp.discrete, d, hipMemcpyHostToDevice);
        }
        const bool valid = member(b, g);
        const double logdet = h_scal[2 * b], zz = h_scal[2 * b + 1];
        double ll;
        const int stt = batch_set_result(N, valid, h_info[b], logdet, zz, &ll);   // (BOSS_E_NOT_PD: PosDefException of this sample's cholesky)
        g->host_res[0] = logdet;
        g->host_res[1] = zz;
        g->fitted = stt == BOSS_OK;
        g->have_dinv = false;
        if (logpdf_out) logpdf_out[b] = ll;
        if (status_out) status_out[b] = stt;
    }
    st->refs.store(S);
    for (int b = 0; b < S; ++b) out[b] = hs[b];
    return BOSS_OK;
}

extern "C" int boss_gp_fit_batch(int device, int kernel, int d, int N, const double* X, const double* y, const double* mean_X,
                                 int mean_stride, const unsigned char* discrete, int S, const double* lengthscales,
                                 const double* amplitudes, const double* noise_stds, boss_gp_t** out, double* logpdf_out,
                                 int* status_out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    for (int b = 0; b < S; ++b) out[b] = nullptr;
    if (kernel < 0 || kernel > 2) return fail(BOSS_E_INVALID, "unknown kernel id");
    if (d < 1 || N < 1 || S < 1 || !X || !y) return fail(BOSS_E_INVALID, "need d >= 1, N >= 1, S >= 1 and non-NULL X, y");
    if (N > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");
    if (!lengthscales || !amplitudes || !noise_stds) return fail(BOSS_E_INVALID, "NULL hyper-parameter array");
    if (mean_X && mean_stride != 0 && mean_stride != N) return fail(BOSS_E_INVALID, "mean_stride must be 0 or N");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    const int Np = round_up(N, PRED_RB);
    const bool small = small_fit_ok(c, N, d);
    std::vector<double> buf, yb(Np, 0.0), h_invlam((size_t)d * S), h_hyp(2 * (size_t)S);
    std::vector<int> valid(S);
    pack_points(buf, X, d, N, Np, discrete);
    std::copy(y, y + N, yb.begin());
    for (int b = 0; b < S; ++b)   // (a failed set is reported, the others are built)
        valid[b] = stage_hyper(d, lengthscales + (size_t)b * d, amplitudes[b], noise_stds[b], &h_invlam[(size_t)b * d], &h_hyp[2 * b]);
    FitBatchSpec sp;
    sp.kernel = kernel;
    sp.d = d;
    sp.N = sp.npts = N;
    sp.ldx = Np;
    sp.S = S;
    sp.zero_slab = small;
    sp.pts = &buf;
    sp.yb = &yb;
    sp.mean_X = mean_X;
    sp.mean_stride = mean_stride;
    sp.discrete = discrete;
    sp.compact_extra = (size_t)S * (d + 2);                  // 1/λ | {α², σ²} of the batch kernels
    auto factor = [&](FitBatchSlab& L, hipStream_t s) {
        double* invlamB = L.cextra;
        double* hypB = invlamB + (size_t)S * d;
        hipError_t e = hipMemcpyAsync(invlamB, h_invlam.data(), sizeof(double) * d * S, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hypB, h_hyp.data(), sizeof(double) * 2 * S, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        if (small)
            hipLaunchKernelGGL(small_fit_batch_kernel, dim3(S), dim3(DIAG_THREADS), SMALL_LDS_BYTES, s, d, N, Np, L.ld, kernel,
                               (const double*)invlamB, (const double*)hypB, (const double*)L.pts, L.Xsc, L.sX, (const double*)L.y,
                               (const double*)L.mean, L.sMean, L.A, L.sA, L.inv16, L.sInv, L.scalB, L.infoB);
        else
            batch_factor_enqueue(c, kernel, d, N, Np, S, L.pts, L.y, (const double*)L.mean, L.sMean, invlamB, hypB, L.Xsc, L.sX, L.A, L.ld,
                                 L.sA, L.inv16, L.sInv, L.scalB, L.infoB);
        L.scatter_invlam = invlamB;
        L.scatter_hyp = hypB;
        return hipSuccess;
    };
    auto member = [&](int b, boss_gp* g) {
        g->amp2 = h_hyp[2 * b];
        for (int k = 0; k < d; ++k) g->host_par[k] = h_invlam[(size_t)b * d + k];
        g->host_par[d] = h_hyp[2 * b];
        g->host_par[d + 1] = h_hyp[2 * b + 1];
        return valid[b] != 0;
    };
    return fit_batch_run(c, sp, factor, member, out, logpdf_out, status_out);
}

// boss_ggp_fit_batch: the S posteriors of a GradientGaussianProcess under S parameter sets (arguments as boss_ggp_loglike_batch) as
// resident handles out of one batched factorisation — gradient_gp.jl:307-329 once per sample of a Bayesian-inference fit.
extern "C" int boss_ggp_fit_batch(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY, int S,
                                  const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                  const double* grad_noise_stds, boss_gp_t** out, double* logpdf_out, int* status_out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    for (int b = 0; b < S; ++b) out[b] = nullptr;
    if (kernel < 0 || kernel > 2) return fail(BOSS_E_INVALID, "unknown kernel id");
    if (d < 1 || n < 1 || S < 1 || !X || !y || !dY) return fail(BOSS_E_INVALID, "need d >= 1, n >= 1, S >= 1 and non-NULL X, y, dY");
    if (d > AUG_MAX_D) return fail(BOSS_E_INVALID, "gradient observations: x_dim above 16 is not supported");
    if ((long long)n * (1 + d) > MAX_ROWS) return fail(BOSS_E_INVALID, "augmented system too large (n (1 + d) > 46080)");
    if (!lengthscales || !amplitudes || !noise_stds || !grad_noise_stds) return fail(BOSS_E_INVALID, "NULL hyper-parameter array");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    const int N = n * (1 + d), Np = round_up(N, PRED_RB), ldx = round_up(n, 64);
    std::vector<double> pts, yb(Np, 0.0);
    pack_points(pts, X, d, n, ldx, nullptr);
    for (int j = 0; j < n; ++j) {                            // `_build_obs_vector` (gradient_gp.jl:288-302), built once for all sets
        yb[j] = y[j];
        for (int l = 0; l < d; ++l) yb[(size_t)n * (1 + l) + j] = dY[(size_t)j * d + l];
    }
    FitBatchSpec sp;
    sp.kernel = kernel;
    sp.d = d;
    sp.N = N;
    sp.npts = n;
    sp.ldx = ldx;
    sp.S = S;
    sp.aug = true;
    sp.pts = &pts;
    sp.yb = &yb;
    std::vector<double> h_par;
    std::vector<int> valid(S);
    auto factor = [&](FitBatchSlab& L, hipStream_t s) {
        h_par.assign(L.sPar * S, 0.0);                       // the members' own blocks, uploaded in place
        for (int b = 0; b < S; ++b)
            valid[b] = ggp_stage_set(d, lengthscales + (size_t)b * d, amplitudes[b], noise_stds[b], grad_noise_stds[b], &h_par[(size_t)b * L.sPar]);
        hipError_t e = hipMemcpyAsync(L.par, h_par.data(), sizeof(double) * L.sPar * S, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        batch_middle_enqueue(c, N, Np, S, L.y, nullptr, 0, L.A, L.ld, L.sA, L.inv16, L.sInv, L.scalB, L.infoB, BatchStage(),
                             [&](int b0, int cnt) {
                                 ProfScope ps(c, "gram");
                                 const long long t64 = Np / 64;
                                 hipLaunchKernelGGL(aug_gram_kernel, dim3((unsigned)(t64 * (t64 + 1) / 2), 1, cnt), dim3(256), 0, c->stream,
                                                    (const double*)L.pts, ldx, d, n, N, Np, kernel, (const double*)(L.par + (size_t)b0 * L.sPar + d),
                                                    (const double*)(L.par + (size_t)b0 * L.sPar), L.sPar, L.A + (size_t)b0 * L.sA, L.ld, L.sA, 0);
                             });
        return hipSuccess;
    };
    auto member = [&](int b, boss_gp* g) {
        const double* p = &h_par[(size_t)b * round_up(d + 4, 8)];
        for (int k = 0; k < d + 3; ++k) g->host_par[k] = p[k];
        g->amp2 = p[d];
        return valid[b] != 0;
    };
    return fit_batch_run(c, sp, factor, member, out, logpdf_out, status_out);
}

// boss_ngp_fit_batch: the S posteriors of a NonstationaryGP under S sets of latent values (arguments as boss_ngp_loglike_batch) as
// resident handles out of one batched factorisation; every member keeps its λ(X), α(X), σ(X) in the slab.
extern "C" int boss_ngp_fit_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete, int S,
                                  const double* lam_X, const double* amp_X, const double* noise_X, const double* mean_X,
                                  int mean_stride, boss_gp_t** out, double* logpdf_out, int* status_out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    for (int b = 0; b < S; ++b) out[b] = nullptr;
    if (d < 1 || N < 1 || S < 1 || !X || !y) return fail(BOSS_E_INVALID, "need d >= 1, N >= 1, S >= 1 and non-NULL X, y");
    if (N > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 observations are not supported");
    if (!lam_X || !amp_X || !noise_X) return fail(BOSS_E_INVALID, "NULL latent-value array");
    if (mean_X && mean_stride != 0 && mean_stride != N) return fail(BOSS_E_INVALID, "mean_stride must be 0 or N");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    const int Np = round_up(N, PRED_RB);
    std::vector<double> pts, yb(Np, 0.0);
    pack_points(pts, X, d, N, Np, discrete);
    std::copy(y, y + N, yb.begin());
    FitBatchSpec sp;
    sp.kernel = KERN_GIBBS;
    sp.d = d;
    sp.N = sp.npts = N;
    sp.ldx = Np;
    sp.S = S;
    sp.gibbs = true;
    sp.pts = &pts;
    sp.yb = &yb;
    sp.mean_X = mean_X;
    sp.mean_stride = mean_stride;
    sp.discrete = discrete;
    sp.sExtra = ((size_t)d + 2) * Np;
    std::vector<double> h_par;
    std::vector<int> valid(S);
    auto factor = [&](FitBatchSlab& L, hipStream_t s) {
        h_par.resize(L.sExtra * S);
        for (int b = 0; b < S; ++b)
            valid[b] = ngp_stage_set(d, N, Np, lam_X + (size_t)b * d * N, amp_X + (size_t)b * N, noise_X + (size_t)b * N, &h_par[(size_t)b * L.sExtra]);
        hipError_t e = hipMemcpyAsync(L.extra, h_par.data(), sizeof(double) * L.sExtra * S, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(L.par, 0, sizeof(double) * L.sPar * S, s);   // (a nonstationary handle has no scalar parameters)
        if (e != hipSuccess) return e;
        batch_middle_enqueue(c, N, Np, S, L.y, (const double*)L.mean, L.sMean, L.A, L.ld, L.sA, L.inv16, L.sInv, L.scalB, L.infoB, BatchStage(),
                             [&](int b0, int cnt) {
                                 ProfScope ps(c, "gram");
                                 const int t64 = Np / 64;
                                 const double* par = L.extra + (size_t)b0 * L.sExtra;
                                 hipLaunchKernelGGL(gibbs_gram_kernel, dim3(t64 * (t64 + 1) / 2, 1, cnt), dim3(256), 0, c->stream, (const double*)L.pts,
                                                    par, par + (size_t)d * Np, par + (size_t)(d + 1) * Np, L.sExtra, L.sExtra, d, N, Np,
                                                    L.A + (size_t)b0 * L.sA, L.ld, L.sA, 0);
                             });
        return hipSuccess;
    };
    auto member = [&](int b, boss_gp*) { return valid[b] != 0; };
    return fit_batch_run(c, sp, factor, member, out, logpdf_out, status_out);
}
