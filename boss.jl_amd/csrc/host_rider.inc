// host_rider.inc — boss_gp_update_acq: one posterior update with the FIRST acquisition of the new posterior riding along
// (rider.hpp; included by bosship.hip).  Replaces, for candidates that do not depend on the posterior (SamplingAM / GridAM,
// src/acquisition_maximizers/sampling.jl:43-57, grid.jl:52-65), the pair  estimate_parameters! -> maximize_acquisition  of one BO
// iteration (src/bo.jl:30-48): boss_gp_update followed by boss_acq_ei.

// Candidates up to which the substitution rides along.  Beyond, the fused prediction kernel (one workgroup per 32 candidates, 0.85 of
// the MFMA peak) behind the update is faster than a rider whose accumulate part has long outgrown what the update leaves idle
// (N = 4096, ms per call, one call / two calls: M = 4096 2.22 / 2.49, M = 8192 3.46 / 3.31); the waiting solve workgroups (one per 32
// candidates, a CU's register file each) must also stay well below the number of CUs.
static int rider_max_m() {
    static const int v = getenv("BOSS_RIDER_MAX_M") ? std::min(8192, atoi(getenv("BOSS_RIDER_MAX_M"))) : 4096;
    return v;
}
static bool rider_off() {
    static const bool v = getenv("BOSS_NO_RIDER") && atoi(getenv("BOSS_NO_RIDER"));
    return v;
}
// K-chunks per block row.  A rider workgroup (eight waves, 224 registers) has its CU to itself, and the accumulate part is bound by
// the MFMA rate of that CU (3.4 µs per 128-column block of one 32-candidate strip): what counts is that the whole launch — one solve
// workgroup per 32 candidates plus strips × chunks accumulate workgroups — is resident in ONE round on the CUs the chain leaves (256
// minus two chain, eight strip workgroups and a few for the update's own kernels).  At 1024 candidates: six chunks (224 workgroups;
// eight chunks = 288 workgroups ran in two rounds, 37 instead of ≈ 21 µs per step at the end of the update).
static int rider_chunks(int nstrips) {
    static const int env = getenv("BOSS_RIDER_CHUNKS") ? atoi(getenv("BOSS_RIDER_CHUNKS")) : 0;
    if (env > 0) return std::min(env, RIDER_MAX_CH);
    static const int max_wgs = getenv("BOSS_RIDER_MAX_WGS") ? atoi(getenv("BOSS_RIDER_MAX_WGS")) : 240;
    const int fit = (max_wgs - nstrips) / nstrips;
    if (fit >= 4) return std::min(RIDER_MAX_CH, fit);
    // more candidates: several rounds whatever the count — chunks small enough to balance them (ms per call at 2048 candidates with
    // 3 / 4 / 6 / 8 chunks: 1.61 / 1.58 / 1.52 / 1.60; at 4096 with 1 / 2 / 3 / 4 / 6: 2.67 / 2.22 / 2.27 / 2.22 / 2.24)
    return nstrips <= 64 ? 6 : 4;
}

// The rider of one update: workspaces reserved BEFORE the update's first launch (a hipMalloc / hipFree inside the update would wait
// for the resident kernels), its step k enqueued on the side stream behind the main stream's step k (RiderReq::step), its tail
// behind the update's last kernel.
struct RiderRun {
    boss_gp* g = nullptr;
    const boss_cand* cd = nullptr;
    double *Csc = nullptr, *V = nullptr, *part = nullptr, *part_ss = nullptr, *part_z = nullptr, *pairs = nullptr;
    size_t part_n = 0;                                       // doubles per parity of the partial-sum slots
    int nstrips = 0, nch = 1, slots = 0;                     // slots: partial sums the previous step left for the block row about to be solved
    const ChainPlan* plan = nullptr;
    bool interleaved = false;
    bool s_only = false;                                     // (boss_debug_rider_replay: the S workgroups alone)
};
static int rider_reserve(RiderRun& r) {
    Ctx* c = r.g->ctx;
    const int Np = r.g->Np, nblk = r.g->nblk, Mp = r.cd->Mp;
    r.nstrips = Mp / 32;
    r.nch = rider_chunks(r.nstrips);
    int rc = ws_reserve(c->csc, sizeof(double) * (size_t)r.g->d * Mp);
    if (rc) return rc;
    rc = ws_reserve(c->vscratch, sizeof(double) * (size_t)r.nstrips * 32 * Np);
    if (rc) return rc;
    const size_t part_n = (size_t)RIDER_MAX_CH * r.nstrips * BLK * 32, blk_n = (size_t)nblk * Mp;
    rc = ws_reserve(c->few, sizeof(double) * (2 * part_n + 2 * blk_n + 2 * (size_t)r.nstrips));
    if (rc) return rc;
    r.Csc = (double*)c->csc.p;
    r.V = (double*)c->vscratch.p;
    r.part = (double*)c->few.p;
    r.part_n = part_n;
    r.part_ss = r.part + 2 * part_n;
    r.part_z = r.part_ss + blk_n;
    r.pairs = r.part_z + blk_n;
    if (!few_done_ensure(c, c->stream)) return fail(BOSS_E_ALLOC, "device allocation failed");
    return BOSS_OK;
}
static void rider_step(RiderRun& r, int k) {
    boss_gp* g = r.g;
    Ctx* c = g->ctx;
    hipStream_t s = c->side_stream;
    const int nblk = g->nblk, Mp = r.cd->Mp;
    const unsigned long long base = r.plan->cbase;
    const unsigned budget = poll_budget_ticks(g->Np);
    if (k == 0) {
        // the first panel solve has started, i.e. the Gram kernel has ended: scaled points and the parameter block are on the device.
        // (The only stream-level gate of the rider: every later step is ordered by its predecessor and waits for its diagonal block itself.)
        hipLaunchKernelGGL(rider_gate_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)(c->sig_panel + SIGW_WDONE), 1, 1, base + 1,
                           g->info, budget, 500);
        hipLaunchKernelGGL(scale_cand_kernel, dim3((Mp + 255) / 256), dim3(256), 0, s, r.cd->Craw, r.Csc, g->invlam, g->discrete_dev, g->d, Mp);
    }
    RiderStep p;
    p.A = g->A;
    p.inv16 = g->inv16;
    p.V = r.V;
    p.part_in = r.part + (size_t)(k & 1) * r.part_n;
    p.part_out = r.part + (size_t)((k + 1) & 1) * r.part_n;
    p.part_ss = r.part_ss;
    p.part_z = r.part_z;
    p.Xsc = g->Xsc;
    p.Csc = r.Csc;
    p.sig = c->sig_panel;
    p.info = g->info;
    p.want = base + 8ull * k + 8;
    p.ld = g->ld;
    p.Np = g->Np;
    p.N = g->N;
    p.Mp = Mp;
    p.d = g->d;
    p.kern = g->kernel;
    p.k = k;
    p.nblk = nblk;
    p.nstrips = r.nstrips;
    p.nslots = r.slots;
    p.budget = budget;
    p.amp2 = g->amp2;
    // E_k: block row k+1 over the blocks [0, k-1) in chunks of cb blocks (k <= 1: the K* tile alone)
    int chunks = 0;
    p.cb = 1;
    if (k + 1 < nblk) {
        const int nb = std::max(0, k - 1), want = std::min(r.nch, std::max(1, nb));
        p.cb = nb > 0 ? (nb + want - 1) / want : 1;
        chunks = nb > 0 ? (nb + p.cb - 1) / p.cb : 1;
    }
    p.nchunks = chunks;
    static const int efirst = getenv("BOSS_RIDER_EFIRST") ? atoi(getenv("BOSS_RIDER_EFIRST")) : 0;
    p.efirst = efirst;
#ifdef BOSS_EXPERIMENTS
    static const int exp_rider = getenv("BOSS_EXP_RIDER") ? atoi(getenv("BOSS_EXP_RIDER")) : 0;
    p.exp = exp_rider;
#endif
    static const int lds_dyn = getenv("BOSS_RIDER_LDS") ? atoi(getenv("BOSS_RIDER_LDS")) : RIDER_LDS_BYTES;
    hipLaunchKernelGGL(rider_step_kernel, dim3(r.nstrips * (1 + (r.s_only ? 0 : chunks))), dim3(RIDER_THREADS), lds_dyn, s, p);
    r.slots = chunks;
}
// behind the update's last launch: moments, EI epilogue and arg-max in one launch (rider_final_kernel), answered through the
// context's pinned block under sequence number res_seq.  mu / var / acq: device arrays (M); mask: device bytes or null
static int rider_tail(RiderRun& r, const RiderReq& rq, const double* mean_s_dev, double* mu, double* var, double* acq,
                      const unsigned char* mask, const EiPar& par, unsigned long long res_seq) {
    boss_gp* g = r.g;
    Ctx* c = g->ctx;
    RiderFinal p;
    p.A = g->A;
    p.V = r.V;
    p.part_ss = r.part_ss;
    p.part_z = r.part_z;
    p.mean_s = mean_s_dev;
    p.mu = mu;
    p.var = var;
    p.acq = acq;
    p.mask = mask;
    p.info = g->info;
    p.host_res = (double*)c->pinned;
    p.gate = c->sig_panel + SIGW_GATE;                       // the update's last kernel has started: the z entries of the last blocks are final
    p.want = rq.end_gate;
    c->few_done_cnt += (unsigned long long)r.nstrips;
    p.done_after = c->few_done_cnt;
    p.res_seq = res_seq;
    p.done = c->few_done;
    p.pairs = r.pairs;
    p.ld = g->ld;
    p.Np = g->Np;
    p.nblk = g->nblk;
    p.M = r.cd->M;
    p.Mp = r.cd->Mp;
    p.budget = poll_budget_ticks(g->Np);
    p.amp2 = g->amp2;
    p.par = par;
    hipLaunchKernelGGL(rider_final_kernel, dim3(r.nstrips), dim3(256), 0, c->side_stream, p);
    HIPCHK(hipGetLastError());
    return BOSS_OK;
}

extern "C" int boss_gp_update_acq(boss_gp_t* g, const double* lengthscale, double amplitude, double noise_std, const double* mean_X,
                                  const boss_cand_t* cand, const double* mean_Xs, double fit_coef, double y_max, int has_best,
                                  double best, const unsigned char* valid_mask, double* logpdf_out, double* mu_out, double* var_out,
                                  double* acq_out, long* argmax_out, double* max_out, int* fused_out) {
    if (fused_out) *fused_out = 0;
    if (!g || !cand) return fail(BOSS_E_INVALID, "NULL argument");
    NOT_FOR_AUG(g);
    int rc = validate_hyper(g->d, lengthscale, amplitude, noise_std);
    if (rc) return rc;
    Ctx* c = g->ctx;
    if (cand->ctx != c) return fail(BOSS_E_INVALID, "candidates and posterior live on different devices");
    if (cand->d != g->d) return fail(BOSS_E_INVALID, "candidate dimension differs from the model's x_dim");
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    const int M = cand->M;
    // device scratch as in boss_acq_ei (P = 1): mu | var | acq | mean | (coefs, ymax unused) | mask
    const size_t nd = (size_t)4 * M + 2;
    rc = ws_reserve(c->acq, sizeof(double) * nd + M);
    if (rc) return rc;
    double* dmu = (double*)c->acq.p;
    double* dvar = dmu + M;
    double* dacq = dvar + M;
    double* dmean = dacq + M;
    unsigned char* dmask = (unsigned char*)(dmu + nd);
    double* hres = (double*)c->pinned;
    const bool constrained = !std::isnan(y_max);            // NaN: `constraints === nothing`; +Inf: a constraint that always holds (factor 1)
    EiPar par;
    {
        const double ym = y_max;
        rc = ei_params(c, s, 1, &fit_coef, constrained ? &ym : nullptr, has_best, best, &par, nullptr, nullptr);
        if (rc) return rc;
    }
    // uploads go to the main stream IN FRONT of the update: whatever the rider runs behind its last gate comes after them
    if (valid_mask) HIPCHK(hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s));
    if (mean_Xs) HIPCHK(hipMemcpyAsync(dmean, mean_Xs, sizeof(double) * M, hipMemcpyHostToDevice, s));
    if (valid_mask || mean_Xs) HIPCHK(hipStreamSynchronize(s));   // (pageable caller buffers)
    static const bool verbose = getenv("BOSS_RIDER_VERBOSE") && atoi(getenv("BOSS_RIDER_VERBOSE"));
    const auto t_h0 = std::chrono::steady_clock::now();
    RiderReq rq;
    RiderRun run;
    run.g = g;
    run.cd = cand;
    run.plan = &rq.plan;
    const bool want_rider = !rider_off() && g->Np / BLK >= 3 && chain_applies(c, g->Np, 1, true) && chain_trail_mode(g->Np / BLK) != 2 &&
                            g->d <= HYP_ARGS_MAX_D && !(g->N <= SMALL_MAX_N) && cand->M <= rider_max_m();
    if (want_rider) {
        rc = rider_reserve(run);
        if (rc) return rc;
        // BOSS_RIDER_INTERLEAVE=1: each step enqueued right behind the main stream's step (the host then alternates between two streams
        // per step, which costs it more per launch than the device gains: the default puts the rider's launches behind the update's)
        static const bool interleave = getenv("BOSS_RIDER_INTERLEAVE") && atoi(getenv("BOSS_RIDER_INTERLEAVE"));
        if (interleave) rq.step = [&run](int k) { rider_step(run, k); };
        else rq.step = [](int) {};
        run.interleaved = interleave;
    }
    rc = gp_update_enqueue(g, lengthscale, amplitude, noise_std, mean_X, want_rider ? &rq : nullptr);
    if (rc) {
        if (want_rider) (void)hipStreamSynchronize(c->side_stream);
        return rc;
    }
    bool riding = want_rider && rq.plan.on && rq.end_gate != 0;
    const unsigned long long seq = ++c->acq_seq;
    const auto t_h1 = std::chrono::steady_clock::now();
    if (riding) {
        if (!run.interleaved)
            for (int k = 0; k < g->nblk; ++k) rider_step(run, k);
        rc = rider_tail(run, rq, mean_Xs ? dmean : nullptr, dmu, dvar, dacq, valid_mask ? dmask : nullptr, par, seq);
        if (rc) {
            (void)gp_finish(g, nullptr);
            (void)hipStreamSynchronize(c->side_stream);
            return rc;
        }
    }
    const auto t_h2 = std::chrono::steady_clock::now();
    rc = gp_finish(g, logpdf_out);
    const auto t_h3 = std::chrono::steady_clock::now();
    if (rc) {
        if (riding) (void)hipStreamSynchronize(c->side_stream);   // (its scratch areas are reused by the next call)
        return rc;
    }
    hipStream_t rs = c->side_stream;                         // the stream the results were produced on
    if (riding && !g->fell_back) {
        volatile unsigned long long* seqw = reinterpret_cast<volatile unsigned long long*>(hres) + 2;
        bool got = false;
        for (unsigned long i = 1;; ++i) {
            if (*seqw == seq) {
                got = true;
                break;
            }
            if ((i & 0x3fff) == 0 && hipStreamQuery(rs) != hipErrorNotReady) break;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (!got) HIPCHK(hipStreamSynchronize(rs));
        // a rider gate that gave up after the update's own kernels had all passed leaves the mark behind: its numbers are void
        int info_now = 0;
        std::memcpy(&info_now, &hres[3], sizeof(int));       // (written by rider_final_kernel in front of the epilogue)
        if (*seqw != seq || info_now != 0) {
            HIPCHK(hipStreamSynchronize(rs));
            riding = false;
        }
    } else if (riding) {
        HIPCHK(hipStreamSynchronize(rs));
        riding = false;
    }
    if (!riding) {
        // the update ran (or was repeated) without the rider: the acquisition the ordinary way, on the main stream
        rs = s;
        rc = predict_enqueue(g, cand, mean_Xs ? dmean : nullptr, dmu, dvar);
        if (rc) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, (const double*)dmu, (const double*)dvar, M, M, par,
                           (const double*)nullptr, (const double*)nullptr, dacq, 0, 1.0, valid_mask ? dmask : nullptr, hres, 0ull,
                           (double*)nullptr, 0L);
        HIPCHK(hipStreamSynchronize(s));
    }
    if (mu_out) HIPCHK(hipMemcpyAsync(mu_out, dmu, sizeof(double) * M, hipMemcpyDeviceToHost, rs));
    if (var_out) HIPCHK(hipMemcpyAsync(var_out, dvar, sizeof(double) * M, hipMemcpyDeviceToHost, rs));
    if (acq_out) HIPCHK(hipMemcpyAsync(acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, rs));
    if (mu_out || var_out || acq_out) HIPCHK(hipStreamSynchronize(rs));
    HIPCHK(hipGetLastError());
    if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
    if (max_out) *max_out = hres[0];
    if (fused_out) *fused_out = riding ? 1 : 0;
    if (verbose) {
        const auto t_h4 = std::chrono::steady_clock::now();
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        std::fprintf(stderr, "[bosship rider] host: update enqueue %.0f us, rider enqueue %.0f us, wait for the update %.0f us, then for the rider %.0f us (fused %d)\n",
                     us(t_h0, t_h1), us(t_h1, t_h2), us(t_h2, t_h3), us(t_h3, t_h4), riding ? 1 : 0);
    }
    return BOSS_OK;
}

// Timing aid (tools/rider_probe.py): step k of the rider launched `reps` times on the otherwise idle device, behind a finished
// boss_gp_update_acq on the same handle and candidates (every word the step waits for has long passed; what it writes is scratch).
// ms_out: average duration of one launch by HIP events.
extern "C" int boss_debug_rider_replay(boss_gp_t* g, const boss_cand_t* cand, int k, int reps, int s_only, double* ms_out) {
    if (!g || !cand || !ms_out || k < 2 || k >= g->nblk || reps < 1) return fail(BOSS_E_INVALID, "bad argument");
    NOT_FOR_KPROG(g);
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    HIPCHK(hipDeviceSynchronize());
    ChainPlan plan;
    plan.cbase = 0;
    RiderRun run;
    run.g = g;
    run.cd = cand;
    run.plan = &plan;
    int rc = rider_reserve(run);
    if (rc) return rc;
    rider_step(run, k - 1);
    const int slots = run.slots;
    run.s_only = s_only != 0;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    rider_step(run, k);
    run.slots = slots;
    HIPCHK(hipEventRecord(e0, c->side_stream));
    for (int i = 0; i < reps; ++i) {
        rider_step(run, k);
        run.slots = slots;
    }
    HIPCHK(hipEventRecord(e1, c->side_stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *ms_out = (double)ms / reps;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return BOSS_OK;
}
