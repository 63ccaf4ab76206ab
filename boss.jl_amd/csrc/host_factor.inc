// host_factor.inc — factorisation schedule (look-ahead, paired panels, batched) and the posterior handle:
// create / update / sync for the three models (included by bosship.hip: one translation unit).

// ------------------------------------------------------------------------------------------
// factorisation driver (shared by the single handle and the batched log-likelihood)
// ------------------------------------------------------------------------------------------

// BOSS_LAUNCH_STAMPS=1 (diagnostics): the host time of every launch of an update goes into a ring; an update that took longer than
// BOSS_STALL_MS (default 2.5) prints where the host spent more than 50 µs between two stamps and when the result arrived — a
// blocked submission (a launch call that does not return) looks different from a late result behind promptly submitted launches.
struct LaunchStamps {
    static constexpr int CAP = 512;
    int n = 0;
    int tag[CAP];
    std::chrono::steady_clock::time_point t[CAP];
    void reset() { n = 0; }
    void add(int what) {
        if (n < CAP) {
            tag[n] = what;
            t[n++] = std::chrono::steady_clock::now();
        }
    }
};
static std::atomic<int> g_stamps_on{-1};                  // -1: not decided yet (environment), 0 / 1
static std::atomic<long long> g_stall_us{2500};
static std::mutex g_stall_mtx;
static std::string g_stall_log;                            // reports since the last boss_debug_stall_report
static bool launch_stamps_on() {
    int v = g_stamps_on.load(std::memory_order_relaxed);
    if (v < 0) {
        v = (getenv("BOSS_LAUNCH_STAMPS") && atoi(getenv("BOSS_LAUNCH_STAMPS"))) ? 1 : 0;
        if (getenv("BOSS_STALL_MS")) g_stall_us.store((long long)(atof(getenv("BOSS_STALL_MS")) * 1000.0));
        g_stamps_on.store(v);
    }
    return v != 0;
}
static thread_local LaunchStamps g_stamps;
#define BOSS_STAMP(what) do { if (launch_stamps_on()) g_stamps.add(what); } while (0)
static void launch_stamps_report(const char* who) {
    if (!launch_stamps_on() || g_stamps.n < 2) return;
    const double stall_ms = g_stall_us.load() / 1000.0;
    const auto now = std::chrono::steady_clock::now();
    auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
    const double total = us(g_stamps.t[0], now);
    if (total < stall_ms * 1000.0) return;
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s took %.0f us from its first launch; launches submitted within %.0f us; gaps > 50 us between stamps:", who, total,
                  us(g_stamps.t[0], g_stamps.t[g_stamps.n - 1]));
    std::string msg = buf;
    for (int i = 1; i < g_stamps.n; ++i) {
        const double d = us(g_stamps.t[i - 1], g_stamps.t[i]);
        if (d > 50.0) {
            std::snprintf(buf, sizeof buf, " [%d -> %d at +%.0f: %.0f us]", g_stamps.tag[i - 1], g_stamps.tag[i], us(g_stamps.t[0], g_stamps.t[i - 1]), d);
            msg += buf;
        }
    }
    if (getenv("BOSS_LAUNCH_STAMPS")) std::fprintf(stderr, "[bosship stall] %s\n", msg.c_str());
    std::lock_guard<std::mutex> lk(g_stall_mtx);
    if (g_stall_log.size() < 8192) g_stall_log += msg + "\n";
}
// diagnostics (not part of include/bosship.h): switch the stamps on / off at run time; fetch and clear the reports
extern "C" int boss_debug_launch_stamps(int on, double stall_ms) {
    if (stall_ms > 0.0) g_stall_us.store((long long)(stall_ms * 1000.0));
    g_stamps_on.store(on ? 1 : 0);
    return BOSS_OK;
}
extern "C" int boss_debug_stall_report(char* buf, int cap) {
    std::lock_guard<std::mutex> lk(g_stall_mtx);
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, g_stall_log.size());
        std::memcpy(buf, g_stall_log.data(), n);
        buf[n] = 0;
    }
    g_stall_log.clear();
    return BOSS_OK;
}

static int sched_small_m() {
    static const int v = getenv("BOSS_SMALL_M") ? atoi(getenv("BOSS_SMALL_M")) : 8;    // block columns left when the two-stream choreography stops paying (flat between 5 and 9: 1.38 ms at N = 4096; 12: 1.40, 3: 1.40)
    return v;
}
static bool sched_no_pairs() {
    static const bool v = getenv("BOSS_NO_PAIRS") && atoi(getenv("BOSS_NO_PAIRS"));
    return v;
}
// The panel chain as resident kernels (chain.hpp): the diagonal blocks are factored by potrf_chain_kernel on its own stream, block
// row k+1 is solved by potrf_strips_kernel on another, the other panel solves follow in lockstep (potrf_follow_kernel) — single
// matrices under the gate-capable look-ahead schedule only.  chain_begin launches the resident kernels and is called BEFORE the
// update's first kernel goes to the main stream: the chain workgroups need whole CUs, and follower workgroups that have settled
// everywhere (waiting for the chain's first panel) would keep them from ever starting; between updates the device is idle.
struct ChainPlan {
    bool on = false;
    unsigned long long cbase = 0, critbase = 0;
    unsigned long long up_want = 0;                          // sig[SIGW_UP] when every resident workgroup of this factorisation has started
    const TrailWork* tab = nullptr;                          // BOSS_CHAIN_TRAIL=4: the size's work table on the device (null: per-step launches)
    const int* tab_off = nullptr;                            // ... and where each step's entries start
};
// Time budget of every wait inside the factorisation's kernels (PollTimer, potrf.hpp), in ticks of the 100 MHz device clock:
// ≈ 20× what an update of this size takes (a chain step of ≈ 45 µs per block column plus the trailing updates at 30 TFLOP/s), at
// least 20 ms.  BOSS_POLL_BUDGET_MS overrides it.
static unsigned poll_budget_ticks(int Np) {
    static const double env_ms = getenv("BOSS_POLL_BUDGET_MS") ? atof(getenv("BOSS_POLL_BUDGET_MS")) : 0.0;
    const double n = Np;
    const double expect_us = (n / BLK) * 45.0 + n * n * n / 3.0 / 30e6;
    double us = std::max(20000.0, 20.0 * expect_us);
    if (env_ms > 0.0) us = env_ms * 1000.0;
    return (unsigned)std::min(us * 100.0, 4.0e9);
}
// The resident chain was given up on a physical device (a wait timed out: its kernels cannot run side by side there — another
// process or tool holds the CUs, or the queues are serialised): off for every context of that device, for the rest of the process.
static std::atomic<bool> g_chain_off[64];
static std::atomic<long> g_fallbacks{0};                   // updates that were repeated on a simpler schedule (gp_finish), process-wide
// diagnostics (tests): fallbacks so far; whether the resident chain has been switched off for `device`
extern "C" int boss_debug_fallbacks(int device, long* n_out, int* chain_off_out) {
    if (n_out) *n_out = g_fallbacks.load();
    if (chain_off_out) *chain_off_out = g_chain_off[device & 63].load() ? 1 : 0;
    return BOSS_OK;
}
static bool chain_applies(const Ctx* c, int Np, int batch, bool gates) {
    const int nblk = Np / BLK;
    // own stream only: the start-up probe covered the library's four streams; a caller's stream (boss_set_stream) would be a fifth
    // on four hardware queues and may share one with the resident kernels, which then wait for a kernel queued behind them.  Not
    // under BOSS_VIRTUAL_DEVICES either (several contexts' streams on one device, same reason).
    // Chain-bound sizes only.  Beyond 8192 rows the update is bound by its trailing updates, not by the panel chain, and their
    // 128×128 tiles (226 registers, two workgroups per CU) cannot be placed beside the two or three waiting column-update
    // workgroups a CU then holds (≥ 470 of them per step from 64 block columns on): the column update waits for a trailing update
    // that cannot start — only the wait budget ended that, on most first updates at N = 8192 with full tiles (measured, round 4).
    static const int np_max = getenv("BOSS_CHAIN_NP_MAX") ? atoi(getenv("BOSS_CHAIN_NP_MAX")) : 8192;
    return c->lookahead && !c->prof_on && gates && c->chain_ok && c->sig_panel && batch == 1 && !sched_no_pairs() && nblk >= 3 && Np <= np_max &&
           c->stream == c->own_stream && virtual_devices() == 0 && !g_chain_off[c->device & 63].load(std::memory_order_relaxed);
}
// Trailing update under the chain (BOSS_CHAIN_TRAIL, see potrf_enqueue): 0 = one main-stream launch per step, 1 = main-stream pairs,
// 2 = the two-stream gated schedule (the only one that uses the side stream while the chain runs), 4 = deferred (trail_plan).
// Measured on MI355X (ms per update, p50, mode 0 / 1 / 4 with its default P, Q): N = 1024: 0.253 / 0.268 / 0.251 (P = 1; 0.259 with
// P = 2), 2048: 0.490–0.495 / 0.512 / 0.479, 4096: 1.102–1.107 / — / 1.067–1.073, 8192: 5.04 / 4.68 / 4.44 — the deferred schedule
// from 16 block columns on, the plain per-step update below.
static int chain_trail_mode(int nblk) {
    static const int env = getenv("BOSS_CHAIN_TRAIL") ? atoi(getenv("BOSS_CHAIN_TRAIL")) : -1;
    return env >= 0 ? env : (nblk < 16 ? 0 : 4);
}
// Panels per far batch of the deferred schedule (BOSS_TRAIL_PANELS, 1 … 8), and how many a unit may still lack when it becomes
// near work (BOSS_TRAIL_LAG, 1 … 8).  Defaults by size (measured, N = 4096: P, Q = 2, 1: 1.067–1.073 ms; 3, 1: 1.085; 2, 2: 1.090;
// 4, 2: 1.130; 1, 1: 1.135; 8, 3: 1.370.  N = 8192: 4, 3: 4.44; 4, 2: 4.47; 3, 1: 4.53; 2, 1: 4.57): short batches where the chain
// period bounds every step, longer ones where the trailing work does.
static int trail_panels(int nblk) {
    static const int v = getenv("BOSS_TRAIL_PANELS") ? atoi(getenv("BOSS_TRAIL_PANELS")) : 0;
    return v > 0 ? std::min(8, v) : (nblk <= 44 ? 2 : 4);
}
static int trail_lag(int nblk) {
    static const int v = getenv("BOSS_TRAIL_LAG") ? atoi(getenv("BOSS_TRAIL_LAG")) : 0;
    return v > 0 ? std::min(8, v) : (nblk <= 44 ? 1 : 3);
}
// Deferred trailing update under the chain (BOSS_CHAIN_TRAIL=4): the work of every step as a table of 32×128 strips, each with the
// run of panels it receives in one pass (TrailWork, potrf_colupd_tab_kernel).  Units: tile (i, j) of block column j = 1 … nblk-1
// (j <= i < nblk) and the δ^T strip of column j (i = nblk).  Tile (j, j) receives panels 0 … j-2 here and panel j-1 from the chain
// kernel, so it must be complete by the end of step j-2; every other unit receives panels 0 … j-1 and must be complete by the end of
// step j-1, before the panel solve of step j reads it.  Step k:
//   near   what the chain and the next panel solve need — tiles (k+2, k+1), (k+2, k+2) first (the eight critical strips, counted
//          into sig[CRIT] as before), then the rest of column k+1 and its δ^T strip — receive every panel they still lack;
//   ahead  tiles (k+3, k+2), (k+3, k+3), critical one step later, are brought up to panel k, so that their critical pass is K = 128;
//   far    the other units of columns >= k+2 receive batches of P pending panels (K = 128·P: C is read and written once per P
//          panels instead of once per panel), least slack first, until the step holds its share of what is left: the remaining
//          work (cost model: P panels of one strip = P + C0 units) spread evenly over the remaining steps.  A unit's slack counts
//          the far steps it has left against the batches it still needs to reach its near step lacking at most Q panels; at no
//          slack it goes out whatever the share (with fewer than P panels if that is all it lacks).  Steps 0 … P-2 have no
//          complete batch yet and carry little far work; the middle steps catch up.
// Panels are applied in ascending order, every (unit, panel) pair exactly once, and the table depends on nblk and P only, so each
// strip's accumulation order is fixed (tests/test_trail_plan.py replays it).
static void trail_plan(int nblk, int P, int Q, std::vector<TrailWork>& out, std::vector<int>& off) {
    constexpr double C0 = 0.7;                               // a strip's C traffic and start-up, in panels (K = 128 strip: 46 µs for 2080 of
                                                             // them at k = 0 against 27.7 µs of MFMA work)
    out.clear();
    off.assign(std::max(nblk, 1), 0);
    if (nblk < 2) return;
    std::vector<int> have((size_t)(nblk + 1) * (nblk + 1), 0);   // have[j*(nblk+1)+i]: panels 0 … have-1 applied to unit (i, j)
    auto H = [&](int i, int j) -> int& { return have[(size_t)j * (nblk + 1) + i]; };
    auto target = [](int i, int j) { return i == j ? j - 1 : j; };
    auto strips = [&](int i) { return i == nblk ? 1 : 4; };
    double cost = 0.0;
    auto emit = [&](int i, int j, int n, bool crit) {
        int& h = H(i, j);
        for (int s = 0; s < strips(i); ++s) out.push_back(TrailWork{i * BLK + 32 * s, j * BLK, h, n | (crit ? 256 : 0)});
        h += n;
        cost += strips(i) * (n + C0);
    };
    for (int k = 0; k + 1 < nblk; ++k) {
        off[k] = (int)out.size();
        double left = 0.0;                                   // what this and the later steps still have to do
        for (int j = k + 1; j < nblk; ++j)
            for (int i = j; i <= nblk; ++i) {
                const int n = target(i, j) - H(i, j);
                if (n > 0) left += strips(i) * (n + C0 * ((n + P - 1) / P));
            }
        const double share = left / (nblk - 1 - k);
        cost = 0.0;
        if (k + 2 < nblk) {
            emit(k + 2, k + 1, k + 1 - H(k + 2, k + 1), true);
            emit(k + 2, k + 2, k + 1 - H(k + 2, k + 2), true);
        }
        for (int i = (k + 2 < nblk ? k + 3 : k + 2); i <= nblk; ++i) emit(i, k + 1, k + 1 - H(i, k + 1), false);
        if (k + 3 < nblk) {
            emit(k + 3, k + 2, k + 1 - H(k + 3, k + 2), false);
            emit(k + 3, k + 3, k + 1 - H(k + 3, k + 3), false);
        }
        // far candidates by slack: the steps left before the unit becomes near work, less the batches it still needs so that it
        // then lacks at most Q panels (the near pass of a late step has few strips: its longest strip is its duration)
        struct Cand {
            int slack, j, i, n;
        };
        std::vector<Cand> cand;
        for (int j = k + 2; j < nblk; ++j)
            for (int i = j; i <= nblk; ++i) {
                if ((i == k + 2 && j == k + 2) || (i == k + 3 && j <= k + 3)) continue;   // near / ahead above
                const int b = k + 1 - H(i, j);                                          // pending panels
                const int steps = (i == j ? j - 2 : j - 1) - k;                         // far steps left, this one included
                const int slack = steps - std::max(0, (b + steps - Q + P - 1) / P);
                if (b >= P || (b > 0 && slack <= 0)) cand.push_back(Cand{slack, j, i, std::min(b, P)});
            }
        std::stable_sort(cand.begin(), cand.end(), [](const Cand& x, const Cand& y) { return x.slack < y.slack; });
        for (const Cand& w : cand) {
            if (w.slack > 0 && cost >= share) break;          // what has no slack left goes out whatever the step's share
            emit(w.i, w.j, w.n, false);
        }
    }
    off[nblk - 1] = (int)out.size();
}
// The size's table on the device, planned and uploaded (behind the main stream's earlier work) on first use; null if it cannot be
// allocated — the update then takes the per-step launches of mode 0
static const TrailWork* trail_table(Ctx* c, int nblk, const int** off) {
    if (nblk < 3 || nblk > 64) return nullptr;
    Ctx::TrailTab& t = c->trail[nblk];
    if (!t.dev) {
        trail_plan(nblk, trail_panels(nblk), trail_lag(nblk), t.host, t.off);
        const size_t bytes = t.host.size() * sizeof(TrailWork);
        if (hipMalloc((void**)&t.dev, bytes) != hipSuccess) {
            (void)hipGetLastError();
            t.dev = nullptr;
            return nullptr;
        }
        if (hipMemcpyAsync(t.dev, t.host.data(), bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(t.dev);
            t.dev = nullptr;
            return nullptr;
        }
    }
    *off = t.off.data();
    return t.dev;
}
static ChainPlan chain_begin(Ctx* c, double* A, int ld, int Np, double* inv16, int* info) {
    ChainPlan p;
    if (!chain_applies(c, Np, 1, true)) return p;
    const int nblk = Np / BLK;
    if (chain_trail_mode(nblk) == 4) p.tab = trail_table(c, nblk, &p.tab_off);   // (before the resident kernels: the upload is a first-use copy)
    p.on = true;
    p.cbase = c->chain_seq;
    c->chain_seq += 8ull * nblk + 16;
    p.critbase = c->crit_seq;
    c->crit_seq += 8ull * (nblk - 2);                        // steps 0 .. nblk-3 deliver eight critical strips each
#ifdef BOSS_EXPERIMENTS
    static const bool drop_chain = getenv("BOSS_EXP_DROP_CHAIN") && atoi(getenv("BOSS_EXP_DROP_CHAIN"));
#else
    constexpr bool drop_chain = false;
#endif
    if (!(drop_chain || c->test_drop_chain)) {
        const unsigned budget = poll_budget_ticks(Np);
        hipLaunchKernelGGL(potrf_chain_kernel, dim3(2), dim3(DIAG_THREADS), CHAIN_LDS_BYTES, c->chain_stream, A, ld, nblk, inv16, info, c->sig_panel,
                           p.cbase, p.critbase, budget);
        // 90 KB of (unused) dynamic LDS per strip workgroup: one per CU, and no bulk-update workgroup (81 KB) beside it — the strips are
        // on the step's critical path and a bulk wave on their SIMD halves their matrix rate
        hipLaunchKernelGGL(potrf_strips_kernel, dim3(8), dim3(TRSM_THREADS), STRIPS_LDS_BYTES, c->strip_stream, A, ld, nblk, (const double*)inv16,
                           c->sig_panel, p.cbase, p.critbase, info, budget);
        c->up_seq += 2 + 8;
        p.up_want = c->up_seq;
    }
    return p;
}
// Main stream, behind the Gram kernel and in front of the first panel solve: ends when every resident workgroup has started
static void chain_ready(Ctx* c, const ChainPlan& p, int Np, int* info) {
    if (!p.on || c->test_drop_chain) return;
    // needed where the first panel solve alone can cover every CU (its (Np - 256)/16 + 1 two-wave workgroups: from ≈ 32 block columns
    // on); below that a chain workgroup always finds its CU
    static const int force = getenv("BOSS_CHAIN_READY") ? atoi(getenv("BOSS_CHAIN_READY")) : -1;
    const int followers = (Np - 2 * BLK) / 16 + 1;
    const bool need = followers + 16 > c->n_cus;
    if (force == 0 || (force < 0 && !need)) return;
    hipLaunchKernelGGL(chain_ready_kernel, dim3(1), dim3(64), 0, c->stream, c->sig_panel, p.up_want, info, poll_budget_ticks(Np));
}
// gates: cross-stream releases by gate / publish kernels are allowed (their timeout marks info with INT_MIN, which only gp_finish
// knows how to recover from: callers without that fallback pass false and get events)
// step_hook (or null; chain schedules 0 and 1 only): called right behind the main-stream launches of every step k — a rider enqueues
// its own step on the side stream there, so that neither stream's launches sit behind the other's in the host's enqueue order
static void potrf_enqueue(Ctx* c, double* A, int ld, int Np, int batch, size_t bstride, double* inv16,
                          size_t inv16_bstride, int* info, bool gates = true, const ChainPlan* plan = nullptr,
                          const std::function<void(int)>* step_hook = nullptr) {
    const int nblk = Np / BLK;
    hipStream_t s = c->stream;
    const unsigned budget = poll_budget_ticks(Np);
    // Beyond 8192 rows the trailing updates run on 128×128 tiles, two workgroups per CU (226 registers each): a column update that is
    // already ON the device and polls for the end of such an update (the gate schedule's publish word) can hold the very registers
    // the update's remaining tiles need — 470 and more waiting workgroups per step from 64 block columns on; measured at N = 12 000:
    // the wait ran into its budget.  There the streams are ordered by events: a waiting kernel is then not dispatched at all.
    if (Np > 8192) gates = false;
    static const int pair_min_batch = getenv("BOSS_PAIR_MIN_BATCH") ? atoi(getenv("BOSS_PAIR_MIN_BATCH")) : 4;
    // small batches keep the two-stream look-ahead below (every launch covers the whole batch in grid.z): their panel
    // chain is still latency-bound and overlaps the trailing updates
    static const int la_batch_max = getenv("BOSS_LA_BATCH_MAX") ? atoi(getenv("BOSS_LA_BATCH_MAX")) : 8;
    const bool la_batch = batch <= la_batch_max && c->lookahead && !c->prof_on && nblk >= 3;
    if (batch >= pair_min_batch && nblk >= 3 && !la_batch) {
        // Batched factorisations have parallelism to spare and are bound by the HBM traffic of the
        // trailing updates (every step reads and writes the whole trailing matrix).  Pair the panels:
        //   diag_k, solve_k, column k+1 <- panel k, diag_{k+1}, solve_{k+1}, trailing(>= k+2) <- panels k,k+1 (K = 256)
        // so each trailing tile moves through HBM half as often.  One stream, no events.
        for (int k = 0; k < nblk; k += 2) {
            for (int kk = k; kk < k + 2 && kk < nblk; ++kk) {
                {
                    ProfScope ps(c, "potrf_diag");
                    hipLaunchKernelGGL(potrf_diag_kernel, dim3(1, 1, batch), dim3(DIAG_THREADS), DIAG_LDS_BYTES, s, A, ld, bstride,
                                       kk, inv16, inv16_bstride, info, (unsigned long long*)nullptr, 0ull);
                }
                const int nrows16 = (Np - (kk + 1) * BLK) / 16 + 1;
                {
                    ProfScope ps(c, "potrf_trsm");
                    hipLaunchKernelGGL(potrf_trsm_kernel, dim3(nrows16, 1, batch), dim3(TRSM_THREADS), 0, s, A, ld, bstride, kk, inv16,
                                       inv16_bstride, (kk + 1) * BLK);
                }
                const int m = nblk - 1 - kk;
                if (kk == k && m > 0) {
                    ProfScope ps(c, "potrf_syrk");
                    hipLaunchKernelGGL(potrf_colupd_kernel, dim3(4 * m + 1, 1, batch), dim3(256), 0, s, A, ld, bstride, kk, m, 1, 0, 1, (unsigned long long*)nullptr, 0ull, info, 0, -1, (unsigned long long*)nullptr, budget);
                }
            }
            const int m2 = nblk - (k + 2);                   // block triangle behind the pair
            if (m2 > 0) {
                ProfScope ps(c, "potrf_syrk");
                hipLaunchKernelGGL(potrf_syrk_kernel<2>, dim3((m2 * (m2 + 1) / 2 + m2) * batch, 1, 1), dim3(256), 0, s, A, ld, bstride,
                                   k, k + 2, m2, batch);
            } else if (m2 == 0 && k + 1 < nblk) {
                // the pair ends the matrix: only the δ^T rows behind it are left (their solve rides in solve_{k+1},
                // but panel k's contribution to the δ^T entries of block column k+1 was applied by colupd) — nothing to do
            }
        }
        return;
    }
    // Look-ahead needs no profiling scopes (they would serialise the two streams) and >= 3 blocks.
    const bool la = c->lookahead && !c->prof_on && nblk >= 3;
    if (la) {
        while ((int)c->ev_panel.size() < nblk) {
            hipEvent_t e0, e1;
            (void)hipEventCreateWithFlags(&e0, hipEventDisableTiming);
            (void)hipEventCreateWithFlags(&e1, hipEventDisableTiming);
            c->ev_panel.push_back(e0);
            c->ev_rest.push_back(e1);
        }
        // (the side stream needs no fork event: everything it runs below waits for a panel event or gate of THIS factorisation)
    }
    const int small_m = sched_small_m();
    const bool no_pairs = sched_no_pairs();
    const bool chain = plan && plan->on;                     // (the resident kernels are already running: chain_begin)
    const unsigned long long cbase = chain ? plan->cbase : 0;
    unsigned long long* const critw = chain ? c->sig_panel + SIGW_CRIT : nullptr;
    auto launch_follow = [&](int kk, unsigned long long gateval) {
        // block row kk+1 belongs to the resident strips: this launch takes the rows below it (and the δ^T strip)
        const int row0 = std::min((kk + 2) * BLK, Np);
        const int nrows16 = (Np - row0) / 16 + 1;
        hipLaunchKernelGGL(potrf_follow_kernel, dim3(nrows16), dim3(TRSM_THREADS), 0, s, A, ld, kk, (const double*)inv16, row0,
                           kk + 1 < nblk ? 1 : 0, c->sig_panel, cbase, gateval, info, budget);
        BOSS_STAMP(1000 + kk);
    };
    int kstart = 0, tail_join = -1;
    unsigned long long pending_sig = 0;                      // wait-value the next diagonal-block kernel has to store (0: none)
    int gated_kk = 0, gated_m3 = 0;                          // the bulk update that waits behind that value
    unsigned long long bulk_pub = 0;                         // value of word bulk_pub_word that says "what the next column update waits for has ended" (0: none)
    int bulk_pub_word = SIGW_BULK;
    unsigned long long far_pub = 0;                          // value of word SIGW_BULK at the end of the last far part / unsplit bulk update
    std::function<void()> flush_gated_bulk = []() {};
    // Chain schedule, trailing update (BOSS_CHAIN_TRAIL): 0 = every step applies its panel to the whole trailing matrix in one launch
    // on the main stream (K = 128); 1 = pairs on the main stream — the even step updates only the next column, the odd step applies
    // both panels to everything (K = 256: half the C-tile traffic, the bound of these launches); 2 = the two-stream schedule below
    // (gated bulk updates beside the chain).  No side stream, gates or publish kernels in modes 0 and 1: nothing that waits is ever
    // on the device beside the chain but the panel solves.
    // Measured on MI355X (round 4, ms per update, modes 0 / 1 / 2): N = 1024: 0.264 / 0.277 / 0.271, 2048: 0.517 / 0.544 / 0.533,
    // 4096: 1.172 / 1.232 / 1.210, 5000: 1.735 / 1.758 / 1.818, 6000: 2.50 / 2.46 / 2.62, 8192: 5.26 / 4.77 / 5.33 — the plain
    // per-step update up to 44 block columns, pairs beyond (their long odd launches hold the chain up at small sizes).
    const int chain_trail = chain_trail_mode(nblk);
    const bool chain_inline = chain && chain_trail != 2;
    // BOSS_CHAIN_PAIRS_UNTIL=p (mode 0 only): pairs for the steps below p — the early, throughput-bound ones —, one launch per step after
    static const int pairs_until_env = getenv("BOSS_CHAIN_PAIRS_UNTIL") ? atoi(getenv("BOSS_CHAIN_PAIRS_UNTIL")) : -1;
    const int pairs_until = chain_trail == 1 ? nblk : (chain_trail == 0 && pairs_until_env > 0 ? pairs_until_env : 0);
    if (chain_inline && pairs_until > 0) {
        int k = 0;
        for (; k + 3 < nblk && k < pairs_until; k += 2) {     // pairs while the odd step still has two block columns below it
            launch_follow(k, 0);
            int m = nblk - 1 - k;
            hipLaunchKernelGGL(potrf_colupd_kernel, dim3(4 * m + 1 + 4, 1, 1), dim3(256), 0, s, A, ld, bstride, k, m, 1, 0, 1,
                               (unsigned long long*)nullptr, 0ull, info, 1, k + 2, critw, budget);
            if (step_hook) (*step_hook)(k);
            launch_follow(k + 1, 0);
            m = nblk - 2 - k;
            hipLaunchKernelGGL(potrf_colupd_kernel, dim3(2 * m * (m + 1) + m, 1, 1), dim3(256), 0, s, A, ld, bstride, k + 1, m, m, 0, 2,
                               (unsigned long long*)nullptr, 0ull, info, 1, -1, critw, budget);
            if (step_hook) (*step_hook)(k + 1);
        }
        kstart = k;
    }
    if (!chain_inline && la && !no_pairs && (batch == 1 || la_batch) && nblk - 1 > small_m + 2) {
        // ---- paired look-ahead: the bulk update applies TWO panels at a time (K = 256: half the trailing-matrix
        // traffic, better tile efficiency, half the events) and has TWO steps of slack:
        //   even step e:  diag, solve,  column e+1 <- panel e                                   (K = 128)
        //   odd  step o:  diag, solve,  [bulk(o-2) done]  columns o+1, o+2 <- panels o-1, o     (K = 256)
        //                 side stream:  bulk(o): columns >= o+3 <- panels o-1, o                 (K = 256)
        // Every column still receives every earlier panel exactly once; the tail (few block columns left)
        // falls through to the single-stream steps below, entered at an even step.
        int last = -1;
        int k = 0;
        // Bulk tiles of 64×128 for a single matrix: workgroups half as long, so the chain kernels that overlap a bulk
        // update get CUs sooner (1.63 against 1.73 ms at N = 4096; BOSS_BULK_HALF=0: 128×128 tiles)
        static const bool half_tiles = !(getenv("BOSS_BULK_HALF") && !atoi(getenv("BOSS_BULK_HALF")));
        // ... and held to ONE workgroup per CU by 81 KB of (unused) dynamic LDS: the bulk then leaves half of every
        // SIMD's registers free, so the solve and the column update of the step it overlaps start at once beside it
        // (they used to wait ≈25 µs for the first bulk tiles to retire — the dispatcher does not steer a kernel's
        // workgroups towards free CUs, profiles/r02_cu_bulkmask_only.log) and the diagonal block (78 KB of LDS, 16 waves)
        // gets the first CU a bulk tile leaves.  Same bulk throughput (89 µs for the first update either way), the
        // overlapped steps 132 instead of 159 µs (profiles/r02_chain_timeline_bulk_one_per_cu.log); BOSS_BULK_LDS=0: off.
        static const int bulk_lds = (getenv("BOSS_BULK_LDS") ? atoi(getenv("BOSS_BULK_LDS")) : 81) * 1024;
        // first: block column the update starts at (kk+3: everything beyond the two columns the column update took)
        auto launch_bulk = [=](int kk, int m3, int first, int skip00) {   // columns >= first <- panels kk-1, kk (K = 256), then its completion event
            if (half_tiles && batch == 1 && Np <= 8192) {     // chain-bound sizes; large systems are bulk-bound: full tiles, two per CU
                hipLaunchKernelGGL((potrf_syrk_kernel<2, true>), dim3(m3 * (m3 + 1) / 2 + m3, 2, 1), dim3(256), bulk_lds, c->side_stream,
                                   A, ld, bstride, kk - 1, first, m3, 0, skip00);
            } else
                hipLaunchKernelGGL(potrf_syrk_kernel<2>, dim3(m3 * (m3 + 1) / 2 + m3, 1, batch), dim3(256), 0, c->side_stream, A, ld,
                                   bstride, kk - 1, first, m3, 0, skip00);
            (void)hipEventRecord(c->ev_rest[kk], c->side_stream);
        };
        // Chain schedule: the bulk update of an odd step o goes out in two parts —
        //   near(o)  columns o+3, o+4 (32×128 strips): what the column update of step o+2 waits for;
        //   far(o)   columns >= o+5: needed by near(o+2), i.e. it has FOUR steps until the chain needs its result.
        // As one kernel the whole update had to end within two steps; with the chain at 28 µs per step the first bulk updates
        // (60-90 µs) did not, and the chain waited for them (profiles/r03_chain_timeline_unsplit_bulk.log).
        // The last pair before the single-stream tail stays in one piece (the tail waits for one word).
        static const bool split_off = getenv("BOSS_NO_BULK_SPLIT") && atoi(getenv("BOSS_NO_BULK_SPLIT"));
        flush_gated_bulk = [&, launch_bulk]() {
            if (!pending_sig) return;
            hipLaunchKernelGGL(potrf_gate_kernel, dim3(1), dim3(64), 0, c->side_stream, c->sig_panel, pending_sig, info, budget);
            const bool last_pair = nblk - 2 - gated_kk <= small_m + 1;
            if (chain && !split_off && !last_pair && gated_m3 > 2) {
                const int kk = gated_kk, m = gated_m3 + 2;    // m block rows below panel kk
                // near part first: columns kk+3 (without its diagonal tile: the column update of step kk took it), kk+4, and tile
                // (kk+5, kk+5) (which the column update of step kk+2 writes next).  Both parts share the side stream — a third
                // stream would share a hardware queue with one of the four the schedule already keeps busy at the same time
                // (GPU_MAX_HW_QUEUES = 4: kernels of streams on one queue run one after the other, and the resident chain would
                // wait for a kernel queued behind it) — so near(o+2) runs behind far(o): far(o) + near(o+2) have four steps.
                hipLaunchKernelGGL(potrf_colupd_kernel, dim3((4 * (m - 2) + 1) + (4 * (m - 3) + 1) + 4, 1, 1), dim3(256), 0, c->side_stream, A, ld,
                                   bstride, kk, m, 2, 2, 2, (unsigned long long*)nullptr, 0ull, info, 1, kk + 5, (unsigned long long*)nullptr, budget);
                bulk_pub = ++c->sig_seq;
                bulk_pub_word = SIGW_NEAR;
                hipLaunchKernelGGL(potrf_publish_kernel, dim3(1), dim3(64), 0, c->side_stream, c->sig_panel + SIGW_NEAR, bulk_pub);
                launch_bulk(kk, gated_m3 - 2, kk + 5, 1);     // far part, without tile (kk+5, kk+5)
                far_pub = ++c->sig_seq;
                hipLaunchKernelGGL(potrf_publish_kernel, dim3(1), dim3(64), 0, c->side_stream, c->sig_panel + SIGW_BULK, far_pub);
            } else {
                launch_bulk(gated_kk, gated_m3, gated_kk + 3, chain ? 1 : 0);
                bulk_pub = ++c->sig_seq;                     // stored (word 3) by a kernel that starts when this bulk update has ended
                bulk_pub_word = SIGW_BULK;
                far_pub = bulk_pub;
                hipLaunchKernelGGL(potrf_publish_kernel, dim3(1), dim3(64), 0, c->side_stream, c->sig_panel + SIGW_BULK, bulk_pub);
            }
            pending_sig = 0;
        };
        for (; k + 1 < nblk; k += 2) {
            if (nblk - 1 - k <= small_m + 1) break;          // tail: switch at an even step
            for (int kk = k; kk < k + 2; ++kk) {
                if (chain) {
                    launch_follow(kk, pending_sig);           // (its entry releases the gated bulk update, as the diagonal-block kernel's did)
                    flush_gated_bulk();
                } else {
                    hipLaunchKernelGGL(potrf_diag_kernel, dim3(1, 1, batch), dim3(DIAG_THREADS), DIAG_LDS_BYTES, s, A, ld, bstride, kk, inv16,
                                       inv16_bstride, info, pending_sig ? c->sig_panel : (unsigned long long*)nullptr, pending_sig);
                    flush_gated_bulk();
                    const int nrows16 = (Np - (kk + 1) * BLK) / 16 + 1;
                    hipLaunchKernelGGL(potrf_trsm_kernel, dim3(nrows16, 1, batch), dim3(TRSM_THREADS), 0, s, A, ld, bstride, kk, inv16, inv16_bstride,
                                       (kk + 1) * BLK);
                }
                const int m = nblk - 1 - kk;
                // chain schedule: tile (kk+1, kk+1) receives panel kk inside the chain kernel; in exchange the column update brings one
                // diagonal tile further down up to date (see potrf_colupd_kernel)
                if (kk == k) {
                    const int xblk = (chain && m >= 2) ? kk + 2 : -1;
                    hipLaunchKernelGGL(potrf_colupd_kernel, dim3(4 * m + 1 + (xblk >= 0 ? 4 : 0), 1, batch), dim3(256), 0, s, A, ld, bstride, kk, m, 1, 0, 1,
                                       (unsigned long long*)nullptr, 0ull, info, chain ? 1 : 0, xblk, critw, budget);
                } else {
                    const bool poll = bulk_pub != 0;          // the previous bulk update went out behind a gate: its end is published
                    if (last >= 0 && !poll) (void)hipStreamWaitEvent(s, c->ev_rest[last], 0);
                    const int nc = m >= 2 ? 2 : 1;
                    const int xblk = (chain && m - 2 > 0) ? kk + 3 : -1;
                    hipLaunchKernelGGL(potrf_colupd_kernel, dim3((4 * m + 1) + (nc == 2 ? 4 * (m - 1) + 1 : 0) + (xblk >= 0 ? 4 : 0), 1, batch), dim3(256), 0, s,
                                       A, ld, bstride, kk, m, nc, 0, 2, poll ? c->sig_panel + bulk_pub_word : (unsigned long long*)nullptr, bulk_pub, info,
                                       chain ? 1 : 0, xblk, critw, budget);
                    const int m3 = m - 2;                     // block triangle beyond the two columns just updated
                    if (m3 > 0) {
                        if (gates && c->sig_panel && batch == 1) {
                            // released by the NEXT diagonal-block kernel's entry (= this column update has finished): no event on the
                            // chain's stream.  The gate and the bulk update are enqueued right BEHIND that kernel (flush_gated_bulk), never
                            // before it: wherever kernels end up serialised in submission order (counter collection under rocprofv3,
                            // HIP_LAUNCH_BLOCKING, a debugger) the gate then finds its word already stored instead of spinning into its timeout.
                            pending_sig = ++c->sig_seq;
                            gated_kk = kk;
                            gated_m3 = m3;
                        } else {
                            (void)hipEventRecord(c->ev_panel[kk], s);
                            (void)hipStreamWaitEvent(c->side_stream, c->ev_panel[kk], 0);
                            launch_bulk(kk, m3, kk + 3, chain ? 1 : 0);
                        }
                        last = kk;
                    }
                }
            }
        }
        // the last bulk update still runs on the side stream; the tail's first diagonal block and panel solve touch
        // only block column k (brought up to date by the column updates above), so the join waits until the tail's
        // first trailing update
        tail_join = last;
        kstart = k;
    }
    int last_rest = tail_join;
    for (int k = kstart; k < nblk; ++k) {
        if (chain) {
            launch_follow(k, pending_sig);
            flush_gated_bulk();
        } else {
            {
                ProfScope ps(c, "potrf_diag");
                hipLaunchKernelGGL(potrf_diag_kernel, dim3(1, 1, batch), dim3(DIAG_THREADS), DIAG_LDS_BYTES, s, A, ld, bstride,
                                   k, inv16, inv16_bstride, info, pending_sig ? c->sig_panel : (unsigned long long*)nullptr, pending_sig);
                flush_gated_bulk();
            }
            const int nrows16 = (Np - (k + 1) * BLK) / 16 + 1;   // rows below + one 16-row group of the RHS block
            {
                ProfScope ps(c, "potrf_trsm");
                hipLaunchKernelGGL(potrf_trsm_kernel, dim3(nrows16, 1, batch), dim3(TRSM_THREADS), 0, s, A, ld, bstride, k, inv16,
                                   inv16_bstride, (k + 1) * BLK);
            }
        }
        const int m = nblk - 1 - k;
        if (m == 0) {
            if (step_hook && chain_inline) (*step_hook)(k);
            break;
        }
        if (la && (m <= small_m + 1 || chain)) {         // (+1: the tail is entered with small_m + 1 columns left — no lone event-ordered step in between)
            // few tiles left: one small single-stream launch beats the two-stream choreography
            const bool poll = last_rest >= 0 && last_rest == tail_join && bulk_pub != 0;   // the paired phase's last bulk update: its end is published
            if (last_rest >= 0 && !poll) (void)hipStreamWaitEvent(s, c->ev_rest[last_rest], 0);
            last_rest = -1;
            if (chain_inline && plan->tab) {                 // deferred schedule: the step's entries of the work table
                const int* off = plan->tab_off;
                hipLaunchKernelGGL(potrf_colupd_tab_kernel, dim3(off[k + 1] - off[k]), dim3(256), 0, s, A, ld, plan->tab + off[k], k, critw);
            } else
                hipLaunchKernelGGL(potrf_colupd_kernel, dim3(2 * m * (m + 1) + m, 1, batch), dim3(256), 0, s, A, ld, bstride, k,
                                   m, m, 0, 1, poll ? c->sig_panel + bulk_pub_word : (unsigned long long*)nullptr, bulk_pub, info, chain ? 1 : 0, -1, critw, budget);
            BOSS_STAMP(2000 + k);
            if (step_hook && chain_inline) (*step_hook)(k);
            continue;
        }
        if (!la) {
            ProfScope ps(c, "potrf_syrk");
            hipLaunchKernelGGL(potrf_syrk_kernel<1>, dim3(m * (m + 1) / 2 + m, 1, batch), dim3(256), 0, s, A, ld, bstride, k,
                               k + 1, m, 0);
            continue;
        }
        // ---- look-ahead: panel chain on `s`, bulk of the trailing update on the side stream ----------
        // the next panel's block column was last written by the side stream's update of step k-1
        {
            const bool poll = last_rest >= 0 && last_rest == tail_join && bulk_pub != 0;
            if (last_rest >= 0 && !poll) (void)hipStreamWaitEvent(s, c->ev_rest[last_rest], 0);
            hipLaunchKernelGGL(potrf_colupd_kernel, dim3(4 * m + 1, 1, batch), dim3(256), 0, s, A, ld, bstride, k, m, 1, 0, 1,
                               poll ? c->sig_panel + bulk_pub_word : (unsigned long long*)nullptr, bulk_pub, info, 0, -1, (unsigned long long*)nullptr, budget);
        }
        last_rest = -1;
#ifdef BOSS_EXPERIMENTS
        static const int exp_norest = getenv("BOSS_EXP_NOREST") ? atoi(getenv("BOSS_EXP_NOREST")) : 0;   // timing experiments only
#else
        constexpr int exp_norest = 0;
#endif
        if (m >= 2 && exp_norest != 1) {
            // the bulk update is released only AFTER the column update has been dispatched, so the two
            // do not fight for CUs; it then overlaps the next diagonal block + panel solve
            const int m2 = m - 1;                             // block triangle beyond the next panel
            (void)hipEventRecord(c->ev_panel[k], s);
            (void)hipStreamWaitEvent(c->side_stream, c->ev_panel[k], 0);
            if (exp_norest != 2)
                hipLaunchKernelGGL(potrf_syrk_kernel<1>, dim3(m2 * (m2 + 1) / 2 + m2, 1, batch), dim3(256), 0, c->side_stream, A,
                                   ld, bstride, k, k + 2, m2, 0);
            (void)hipEventRecord(c->ev_rest[k], c->side_stream);
            last_rest = k;
        }
    }
    if (la && last_rest >= 0) (void)hipStreamWaitEvent(s, c->ev_rest[last_rest], 0);   // join
}

static void gram_enqueue(Ctx* c, const double* Xsc, size_t xs_bstride, int d, int N, int Np, int kern,
                         const double* hyp, double* A, int ld, size_t bstride, int batch) {
    ProfScope ps(c, "gram");
    const int nt = Np / 64;
    hipLaunchKernelGGL(gram_kernel, dim3(nt * (nt + 1) / 2, 1, batch), dim3(256), 0, c->stream, Xsc, xs_bstride, d, N,
                       Np, kern, hyp, A, ld, bstride, 0);
}

// ------------------------------------------------------------------------------------------
// posterior handle
// ------------------------------------------------------------------------------------------
static void gp_release(boss_gp* g) {
    if (!g) return;
    if (g->ctx) (void)hipSetDevice(g->ctx->device);
    if (g->ctx) chain_quiesce(g->ctx);                       // the resident chain kernels of a last update may still be winding down
    if (g->set) {
        // a member of a batch-fitted set: its arrays are views into the set's slab, which goes with the last member
        if (g->ctx) (void)hipStreamSynchronize(g->ctx->stream);
        if (g->dinv_pending && g->ctx) (void)hipStreamSynchronize(g->ctx->side_stream);
        boss_gpset* st = g->set;
        if (st->refs.fetch_sub(1) == 1) {
            gpset_release_storage(st);
            delete st;
        }
        g->Xraw = g->Xsc = g->y = g->mean = g->A = g->inv16 = g->Dinv = g->Dinv2 = g->invlam = g->scal = nullptr;
        g->lamX = g->ampX = g->noiseX = nullptr;
        g->host_res = g->host_par = nullptr;
        g->set = nullptr;
    }
    void* ptrs[] = {g->Xraw, g->Xsc, g->y, g->mean, g->A, g->inv16, g->Dinv, g->Dinv2, g->LT, g->DT2, g->avec, g->invlam, g->scal, g->discrete_dev};   // hyp, info live inside invlam, scal
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (g->host_res) (void)hipHostFree(g->host_res);
    if (g->Winv) (void)hipFree(g->Winv);
    if (g->Linv) (void)hipFree(g->Linv);
    if (g->W2) (void)hipFree(g->W2);
    if (g->prune_a) (void)hipFree(g->prune_a);
    if (g->lamX) (void)hipFree(g->lamX);
    if (g->ampX) (void)hipFree(g->ampX);
    if (g->noiseX) (void)hipFree(g->noiseX);
    if (g->host_par) (void)hipHostFree(g->host_par);
    delete g->kp;
    if (g->par_ev) (void)hipEventDestroy(g->par_ev);
    if (g->dinv_ev) (void)hipEventDestroy(g->dinv_ev);
    delete g;
}

static void pack_points(std::vector<double>& dst, const double* X, int d, int n, int ldp,
                        const unsigned char* discrete) {
    // X is d×n column-major (point-contiguous); dst is [d][ldp] (dimension-major), padding = 0.
    dst.assign((size_t)d * ldp, 0.0);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < d; ++k) {
            double v = X[(size_t)j * d + k];
            if (discrete && discrete[k]) v = std::nearbyint(v);   // Julia round(): half-to-even (kernels.jl:56-59)
            dst[(size_t)k * ldp + j] = v;
        }
}

// npts points of dimension d carrying N observations (N = npts for the plain model, npts (1 + d) with
// gradient observations); y holds the N observed values in the posterior's own ordering.
static int gp_create_common(int device, int kernel, int d, int npts, int N, const double* X, const double* y,
                            const unsigned char* discrete, bool aug, boss_gp_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (kernel < 0 || kernel > 2) return fail(BOSS_E_INVALID, "unknown kernel id");
    if (d < 1 || N < 1 || !X || !y) return fail(BOSS_E_INVALID, "need d >= 1, N >= 1 and non-NULL X, y");
    if (N > MAX_ROWS) return fail(BOSS_E_INVALID, "more than 46080 rows (observations, or n (1 + d) with gradients) are not supported");
    Ctx* c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    boss_gp* g = new boss_gp();
    g->ctx = c;
    g->kernel = kernel;
    g->d = d;
    g->N = N;
    g->Np = round_up(N, PRED_RB);                 // whole 256-row prediction steps (padding = identity)
    g->nblk = g->Np / BLK;
    g->ld = g->Np + RHS_ROWS;
    g->aug = aug;
    g->npts = npts;
    g->nhead = npts;
    g->ldx = aug ? round_up(npts, 64) : g->Np;
    const size_t Np = g->Np, ldx = g->ldx;
#define GALLOC(ptr, bytes)                                        \
    do {                                                          \
        hipError_t e_ = dev_malloc((void**)&(ptr), (bytes));       \
        if (e_ != hipSuccess) {                                   \
            gp_release(g);                                        \
            return fail(BOSS_E_ALLOC, "device allocation failed"); \
        }                                                         \
    } while (0)
    GALLOC(g->Xraw, sizeof(double) * d * ldx);
    GALLOC(g->Xsc, sizeof(double) * d * ldx);
    GALLOC(g->y, sizeof(double) * Np);
    GALLOC(g->mean, sizeof(double) * Np);
    GALLOC(g->A, sizeof(double) * (size_t)g->ld * Np);
    GALLOC(g->inv16, sizeof(double) * g->nblk * 8 * 256);
    GALLOC(g->Dinv, sizeof(double) * g->nblk * BLK * BLK);
    GALLOC(g->Dinv2, sizeof(double) * (g->Np / PRED_RB) * PRED_RB * PRED_RB);
    GALLOC(g->invlam, sizeof(double) * (d + 4));          // 1/(λ+1e-8) | hyp[4]: one upload per update
    g->hyp = g->invlam + d;
    GALLOC(g->scal, sizeof(double) * 4);                  // logdet, zᵀz | info: one download per update
    g->info = (int*)(g->scal + 2);
    if (hipHostMalloc((void**)&g->host_res, 512, hipHostMallocDefault) != hipSuccess ||   // [0,3): logdet, zᵀz, info; [8, 8+d+2): Σ-vector of the small-N likelihood gradient
        hipHostMalloc((void**)&g->host_par, sizeof(double) * (d + 4), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&g->par_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->dinv_ev, hipEventDisableTiming) != hipSuccess ||
        hipHostGetDevicePointer((void**)&g->host_res_dev, g->host_res, 0) != hipSuccess) {
        gp_release(g);
        return fail(BOSS_E_ALLOC, "pinned allocation failed");
    }
    std::memset(g->host_res, 0, 512);                        // (the polled sequence words start from a known value)
    if (discrete) {
        g->discrete.assign(discrete, discrete + d);
        bool any = false;
        for (int k = 0; k < d; ++k) any |= discrete[k] != 0;
        if (any) {
            GALLOC(g->discrete_dev, d);
            (void)hipMemcpy(g->discrete_dev, discrete, d, hipMemcpyHostToDevice);
        } else {
            g->discrete.clear();
        }
    }
#undef GALLOC
    std::vector<double> buf;
    pack_points(buf, X, d, npts, (int)ldx, g->discrete.empty() ? nullptr : g->discrete.data());
    std::vector<double> yb(Np, 0.0);
    std::copy(y, y + N, yb.begin());
    {
        std::lock_guard<std::mutex> lk(c->mtx);              // the device's stream is shared with the other handles
        hipError_t e = hipMemcpyAsync(g->Xraw, buf.data(), sizeof(double) * d * ldx, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(g->y, yb.data(), sizeof(double) * Np, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->mean, 0, sizeof(double) * Np, c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->A, 0, sizeof(double) * (size_t)g->ld * Np, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // host staging buffers go out of scope
        if (e != hipSuccess) {
            gp_release(g);                                   // nothing of a half-built handle stays behind
            return fail(BOSS_E_NO_DEVICE, std::string("uploading the observations: ") + hipGetErrorString(e));
        }
    }
    *out = g;
    return BOSS_OK;
}

extern "C" int boss_gp_create(int device, int kernel, int d, int N, const double* X, const double* y,
                              const unsigned char* discrete, boss_gp_t** out) {
    return gp_create_common(device, kernel, d, N, N, X, y, discrete, false, out);
}

// GradientGaussianProcess (src/models/gradient_gp.jl): dY is d×n column-major, dY[l + d*j] = ∂y/∂x_l at x_j.
extern "C" int boss_ggp_create(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY,
                               boss_gp_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || n < 1 || !X || !y || !dY) return fail(BOSS_E_INVALID, "need d >= 1, n >= 1 and non-NULL X, y, dY");
    if (d > AUG_MAX_D) return fail(BOSS_E_INVALID, "gradient observations: x_dim above 16 is not supported");
    if ((long long)n * (1 + d) > MAX_ROWS) return fail(BOSS_E_INVALID, "augmented system too large (n (1 + d) > 46080)");
    // `_build_obs_vector` (gradient_gp.jl:288-302): [y_1..n, ∂y/∂x_1 (1..n), …, ∂y/∂x_d (1..n)]
    std::vector<double> yt((size_t)n * (1 + d));
    for (int j = 0; j < n; ++j) {
        yt[j] = y[j];
        for (int l = 0; l < d; ++l) yt[(size_t)n * (1 + l) + j] = dY[(size_t)j * d + l];
    }
    return gp_create_common(device, kernel, d, n, n * (1 + d), X, yt.data(), nullptr, true, out);
}

#define NOT_FOR_KPROG(g)                                                                                               \
    do {                                                                                                               \
        if ((g)->kprog) return fail(BOSS_E_INVALID, "not available for program-kernel posteriors (boss_kgp_create)");     \
    } while (0)

// entry points of the plain model that program-kernel posteriors share (boss_gp_update)
#define NOT_FOR_MODELS(g)                                                                                         \
    do {                                                                                                          \
        if ((g)->aug) return fail(BOSS_E_INVALID, "not available for gradient-observation posteriors (boss_ggp_*)"); \
        if ((g)->gibbs) return fail(BOSS_E_INVALID, "not available for nonstationary posteriors (boss_ngp_*)");      \
    } while (0)

// the gradient entry points: a program-kernel posterior is refused unless boss_kgp_set_grad switched its gradients on
#define KPROG_NEEDS_GRAD(g)                                                                                                      \
    do {                                                                                                                         \
        if ((g)->kprog && !(g)->kgrad)                                                                                           \
            return fail(BOSS_E_INVALID, "not available for program-kernel posteriors (boss_kgp_create) without boss_kgp_set_grad"); \
    } while (0)

// appends, reserve and tracked candidates: a program-kernel posterior is refused unless boss_kgp_set_sequential switched them on
#define KPROG_NEEDS_SEQ(g)                                                                                                             \
    do {                                                                                                                               \
        if ((g)->kprog && !(g)->kseq)                                                                                                  \
            return fail(BOSS_E_INVALID, "not available for program-kernel posteriors (boss_kgp_create) without boss_kgp_set_sequential"); \
    } while (0)

#define NOT_FOR_AUG(g)      \
    do {                    \
        NOT_FOR_MODELS(g);  \
        NOT_FOR_KPROG(g);   \
    } while (0)

// entry points that take gradient-observation posteriors but not (yet) nonstationary ones; the former have no prior mean
#define NOT_FOR_GIBBS_MODEL(g, mean_a, mean_b)                                                                      \
    do {                                                                                                            \
        if ((g)->gibbs) return fail(BOSS_E_INVALID, "not available for nonstationary posteriors (boss_ngp_*)");        \
        if ((g)->aug && ((mean_a) || (mean_b)))                                                                      \
            return fail(BOSS_E_INVALID, "gradient-observation posteriors take no prior mean (gradient_gp.jl:307-361)"); \
    } while (0)
#define NOT_FOR_GIBBS(g, mean_a, mean_b)           \
    do {                                           \
        NOT_FOR_KPROG(g);                          \
        NOT_FOR_GIBBS_MODEL(g, mean_a, mean_b);    \
    } while (0)

// NonstationaryGP (src/models/nonstationary_gp/nonstationary_gp.jl): the data of one output slice; the
// per-point hyper-parameters arrive with boss_ngp_update.
extern "C" int boss_ngp_create(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                               boss_gp_t** out) {
    int rc = gp_create_common(device, KERN_SQEXP, d, N, N, X, y, discrete, false, out);
    if (rc) return rc;
    boss_gp* g = *out;
    g->gibbs = true;
    g->kernel = KERN_GIBBS;
    const size_t Np = g->Np;
    if (dev_malloc((void**)&g->lamX, sizeof(double) * d * Np) != hipSuccess ||
        dev_malloc((void**)&g->ampX, sizeof(double) * Np) != hipSuccess ||
        dev_malloc((void**)&g->noiseX, sizeof(double) * Np) != hipSuccess) {
        gp_release(g);
        *out = nullptr;
        return fail(BOSS_E_ALLOC, "device allocation failed");
    }
    return BOSS_OK;
}

// A candidate batch that rides along the factorisation (host_rider.inc): factor_enqueue fills in what the rider's gates need.
struct RiderReq {
    ChainPlan plan;
    unsigned long long end_gate = 0;                         // value of sig[SIGW_GATE] the update's last kernel stores at its entry
    std::function<void(int)> step;                           // enqueues the rider's step k (called behind the main stream's step k)
};
static int gp_finish(boss_gp* g, double* logpdf_out);
static int factor_enqueue(boss_gp* g, RiderReq* rider = nullptr);
static int gp_own(boss_gp* g);

// log marginal likelihood of N observations from log|K| and zᵀz
constexpr double LOG_2PI = 1.8378770664093453;
static double loglik(int N, double logdet, double zz) { return -0.5 * (N * LOG_2PI + logdet + zz); }

// N <= 128 and few dimensions: the one-workgroup kernels (small_calls.hpp) take the plain model's fit, likelihood gradient and
// prediction in one launch each.  BOSS_NO_SMALL_FIT=1 sends them through the tiled kernels; profiling wants its scopes.
static bool small_fit_ok(const Ctx* c, int N, int d) {
    static const bool small_off = getenv("BOSS_NO_SMALL_FIT") && atoi(getenv("BOSS_NO_SMALL_FIT"));
    return N <= SMALL_MAX_N && d <= SMALL_MAX_D && !c->prof_on && !small_off;
}

// What a new factorisation of the handle's data under new hyper-parameters makes stale (every model's update).  The appends
// keep part of it on purpose — the epoch, and have_winv over a rank-one append — and clear their own list (gp_invalidate_append).
static void gp_invalidate(boss_gp* g) {
    g->fitted = false;
    g->have_dinv = false;
    g->have_winv = false;
    g->few_calls = 0;
    g->have_lt = false;
    g->fell_back = false;
    ++g->epoch;
    g->append_calls = 0;
}
// What new observations under unchanged hyper-parameters make stale (every model's append).  keep_inverses: a rank-one append
// patches the resident inverse factors itself.
static void gp_invalidate_append(boss_gp* g, bool keep_inverses) {
    g->fitted = false;
    g->have_lt = false;
    ++g->factor_gen;                                         // every append changes the factor: a block 0 of Dinv built on its own before it is stale
    if (!keep_inverses) {
        g->have_dinv = false;
        g->have_winv = false;
        g->few_calls = 0;
    }
    g->append_path = 0;
}

// A pending update is finished (its error is the caller's), then the handle must hold a valid factorisation.  Caller holds the
// context's lock.
static int gp_settle(boss_gp* g, const char* unfitted = "handle has no valid factorisation") {
    if (g->pending) {
        int rc = gp_finish(g, nullptr);
        if (rc) return rc;
    }
    if (!g->fitted) return fail(BOSS_E_NOT_FITTED, unfitted);
    return BOSS_OK;
}

// What was just enqueued becomes the handle's pending update; waited for unless the caller defers that (boss_gp_sync)
static int update_finish(boss_gp* g, int flags, double* logpdf_out) {
    HIPCHK(hipGetLastError());
    g->pending = true;
    if (flags & BOSS_FIT_NO_SYNC) return BOSS_OK;
    return gp_finish(g, logpdf_out);
}

extern "C" int boss_gp_set_y(boss_gp_t* g, const double* y) {
    if (!g || !y) return fail(BOSS_E_INVALID, "NULL argument");
    if (g->aug) return fail(BOSS_E_INVALID, "not available for gradient-observation posteriors (boss_ggp_*)");
    HIPCHK(hipSetDevice(g->ctx->device));
    std::lock_guard<std::mutex> lk(g->ctx->mtx);
    if (g->pending) (void)gp_finish(g, nullptr);            // an enqueued update still reads the old observations
    {
        int rc = gp_own(g);                                  // (a member of a batch-fitted set shares y with its siblings)
        if (rc) return rc;
    }
    HIPCHK(hipMemcpyAsync(g->y, y, sizeof(double) * g->N, hipMemcpyHostToDevice, g->ctx->stream));
    HIPCHK(hipStreamSynchronize(g->ctx->stream));
    g->fitted = false;
    return BOSS_OK;
}

// gaussian_process.jl:227-229: negative values signal an error (zero is lifted to 1e-8), and so does a NaN.  Null: the set is valid.
static const char* hyper_fault(int d, const double* lam, double amp, double sig) {
    for (int k = 0; k < d; ++k)
        if (!(lam[k] >= 0.0)) return "lengthscales must be >= 0";
    if (!(amp >= 0.0)) return "amplitude must be >= 0";
    if (!(sig >= 0.0)) return "noise_std must be >= 0";
    return nullptr;
}
static int validate_hyper(int d, const double* lam, double amp, double sig) {
    if (!lam) return fail(BOSS_E_INVALID, "lengthscale is NULL");
    const char* why = hyper_fault(d, lam, amp, sig);
    return why ? fail(BOSS_E_INVALID, why) : BOSS_OK;
}
// The parameters as the kernels take them, +1e-8 on each (gaussian_process.jl:239-241): invlam[k] = 1/(λ_k + 1e-8),
// hyp = {(α + 1e-8)², (σ + 1e-8)²}.  False: the set is invalid (hyper_fault) and staged as all-ones — a batch factorises it with
// the others and reports it.
static bool stage_hyper(int d, const double* lam, double amplitude, double noise_std, double* invlam, double* hyp) {
    const bool ok = !hyper_fault(d, lam, amplitude, noise_std);
    for (int k = 0; k < d; ++k) invlam[k] = 1.0 / ((ok ? lam[k] : 1.0) + MIN_PARAM_VALUE);
    const double amp = (ok ? amplitude : 1.0) + MIN_PARAM_VALUE, sig = (ok ? noise_std : 1.0) + MIN_PARAM_VALUE;
    hyp[0] = amp * amp;
    hyp[1] = sig * sig;
    return ok;
}

static int gp_finish(boss_gp* g, double* logpdf_out) {
    Ctx* c = g->ctx;
    if (g->res_polled) {
        // The last kernel of the update writes its results and then this update's sequence number into mapped host memory: the
        // host polls that word — the stream's own completion signal reaches the host 10-20 µs later, which is most of a small
        // update.  (Every later consumer of the factor is ordered behind the update on its stream; a failed launch or a device
        // fault shows up in hipStreamQuery and the wait falls back to the synchronisation.)
        volatile unsigned long long* seq = reinterpret_cast<volatile unsigned long long*>(g->host_res + 3);
        bool got = false;
        static const bool watch = getenv("BOSS_DEBUG_WATCH") && atoi(getenv("BOSS_DEBUG_WATCH"));   // diagnostics: where does a stuck update stand?
        auto t_watch = std::chrono::steady_clock::now();
        for (unsigned long i = 1;; ++i) {
            if (*seq == g->res_seq) {
                got = true;
                break;
            }
            if ((i & 0x3fff) == 0) {
                const hipError_t q = hipStreamQuery(c->stream);
                if (q != hipErrorNotReady) {
                    if (watch) std::fprintf(stderr, "[bosship watch] hipStreamQuery returned %d (%s) before the result word arrived\n", (int)q, hipGetErrorString(q));
                    break;
                }
            }
            if (watch && (i & 0xfffff) == 0 && std::chrono::steady_clock::now() - t_watch > std::chrono::seconds(2) && c->sig_panel) {
                t_watch = std::chrono::steady_clock::now();
                std::fprintf(stderr, "[bosship watch] still waiting for the update's result word\n");
                unsigned long long w[SIG_WORDS];
                int inf = 0;
                (void)hipMemcpy(w, c->sig_panel, sizeof w, hipMemcpyDeviceToHost);
                (void)hipMemcpy(&inf, g->info, sizeof inf, hipMemcpyDeviceToHost);
                const unsigned long long cb = c->chain_seq - (8ull * g->nblk + 16);
                std::fprintf(stderr, "[bosship watch] nblk %d info %d | up %llu/%llu wdone %lld panel %lld (block %lld panel %lld) crit %lld | gate %llu/%llu near %llu bulk %llu | strips",
                             g->nblk, inf, w[SIGW_UP], c->up_seq, (long long)(w[SIGW_WDONE] - cb), (long long)(w[SIGW_PANEL] - cb), (long long)((w[SIGW_PANEL] - cb) / 8),
                             (long long)((w[SIGW_PANEL] - cb) % 8), (long long)(w[SIGW_CRIT] - (c->crit_seq - 8ull * (g->nblk - 2))), w[SIGW_GATE], c->sig_seq,
                             w[SIGW_NEAR], w[SIGW_BULK]);
                for (int q = 0; q < 8; ++q) std::fprintf(stderr, " %lld", (long long)(w[SIGW_PROG + SIGW_PROG_STRIDE * q] - cb));
                std::fprintf(stderr, "\n");
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        g->res_polled = false;
        if (!got) {
            HIPCHK(hipStreamSynchronize(c->stream));
            if (*seq != g->res_seq) {
                // the stream drained without the result word (a kernel of the call did not run): never hand out the previous call's numbers
                g->pending = false;
                g->fitted = false;
                if (c->few_done) (void)hipMemset(c->few_done, 0, sizeof(unsigned long long));
                c->few_done_cnt = 0;
                if (logpdf_out) *logpdf_out = -std::numeric_limits<double>::infinity();
                HIPCHK(hipGetLastError());
                return fail(BOSS_E_NO_DEVICE, "the update's last kernel did not deliver its result (device error)");
            }
        }
    } else {
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    g->pending = false;
    const double logdet = g->host_res[0], zz = g->host_res[1];
    int info;
    std::memcpy(&info, &g->host_res[2], sizeof(int));
    if (info != 0 || !std::isfinite(logdet) || !std::isfinite(zz)) {
        g->fitted = false;
        if (logpdf_out) *logpdf_out = -std::numeric_limits<double>::infinity();
        if (info == INT_MIN) {
            // A wait inside the factorisation gave up (PollTimer): something keeps kernels of different streams from running side by
            // side.  Two steps down, each taken at most once:  (1) the update ran under the resident chain -> the chain is switched off
            // for this physical device (every context, rest of the process) and the update is repeated under gates;  (2) it ran under
            // gates alone -> this context orders its streams with events from now on, and the update is repeated once more.
            const bool drop_chain = g->chained;
            if (drop_chain || g->gated) {                    // (gated: another handle's fallback may already have torn the signal words down)
                (void)hipDeviceSynchronize();
                int code = 0;
                (void)hipMemcpyFromSymbol(&code, HIP_SYMBOL(boss::g_giveup), sizeof(int));
                const int zero = 0;
                (void)hipMemcpyToSymbol(HIP_SYMBOL(boss::g_giveup), &zero, sizeof(int));
                static std::atomic<int> warned{0};
                if ((warned.fetch_add(1) < 2 && !getenv("BOSS_QUIET")) || getenv("BOSS_CHAIN_VERBOSE"))
                    std::fprintf(stderr, "[bosship] device %d: a cross-stream wait gave up (code %d, detail %d) — %s for the rest of the process "
                                 "(results are unaffected; updates of single matrices run slower)\n", c->device, code / 1000, code % 1000,
                                 drop_chain ? "the resident panel chain is switched off on this device" : "this context falls back to event-ordered kernels");
                if (drop_chain) {
                    g_chain_off[c->device & 63].store(true, std::memory_order_relaxed);
                } else {
                    if (c->sig_panel && !c->sig_panel_host) (void)hipFree(c->sig_panel);   // (watch mode: mapped host memory the watcher thread keeps reading — left alone)
                    c->sig_panel = nullptr;
                }
                g->dinv_used = g->dinv_used_prev;            // the repeated update builds the inverses the first attempt would have
                g->fell_back = true;                         // (whatever rode along the first attempt is void)
                g_fallbacks.fetch_add(1);
                int rc = factor_enqueue(g);
                if (rc) return rc;
                g->pending = true;
                return gp_finish(g, logpdf_out);
            }
            return fail(BOSS_E_NO_DEVICE, "look-ahead gate timed out: a kernel of the factorisation never started (device error)");
        }
        char msg[160];
        std::snprintf(msg, sizeof msg, "matrix is not positive definite (pivot %d failed) — PosDefException", info);
        return fail(BOSS_E_NOT_PD, msg);
    }
    g->fitted = true;
    if (logpdf_out) *logpdf_out = loglik(g->N, logdet, zz);
    launch_stamps_report("an update");
    return BOSS_OK;
}

// Dense inverses of the diagonal blocks (prediction operands): 128×128 (Dinv) and 256×256 (Dinv2,
// lower-left quadrant = −C⁻¹ (B A⁻¹)).  Built right after a factorisation on the side stream, so it
// overlaps the log-det reduction, the result copies and the host's return to the caller; the first
// prediction waits on dinv_ev.  (While profiling it runs lazily on the main stream instead.)
static void dinv_launch(boss_gp* g, hipStream_t s, const SetBatch& B = SetBatch()) {
    hipLaunchKernelGGL(potrf_dinv_kernel, dim3(8, g->nblk, B.nb), dim3(64), 0, s, g->A, g->ld, B.sA, g->inv16, B.sInv16, g->Dinv,
                       B.sDinv);
    const int npair = g->Np / PRED_RB;
    const size_t s2 = (size_t)PRED_RB * PRED_RB, s1 = (size_t)2 * BLK * BLK;
    double* T1 = g->Dinv2 + (size_t)BLK * PRED_RB;                         // upper-right quadrant as scratch
    hipLaunchKernelGGL(small_gemm128_kernel, dim3(16, npair, B.nb), dim3(256), 0, s, g->A + BLK, g->ld,
                       (size_t)PRED_RB * ((size_t)g->ld + 1), g->Dinv, BLK, s1, T1, PRED_RB, s2, 1.0, B.sA, B.sDinv, B.sDinv2);
    hipLaunchKernelGGL(small_gemm128_kernel, dim3(16, npair, B.nb), dim3(256), 0, s, g->Dinv + (size_t)BLK * BLK, BLK, s1,
                       (const double*)T1, PRED_RB, s2, g->Dinv2 + BLK, PRED_RB, s2, -1.0, B.sDinv, B.sDinv2, B.sDinv2);
    hipLaunchKernelGGL(dinv_pair_assemble_kernel, dim3(PRED_RB, npair, B.nb), dim3(256), 0, s, (const double*)g->Dinv, g->Dinv2, B.sDinv,
                       B.sDinv2);
}

// The block inverses on the side stream.  gate_value != 0: behind a gate that the kernel just launched on the main stream releases
// at its entry (enqueued after that kernel, see flush_gated_bulk in potrf_enqueue); 0: behind an event recorded on the main stream now.
static void dinv_eager(boss_gp* g, unsigned long long gate_value = 0) {
    Ctx* c = g->ctx;
    if (c->prof_on) return;                                  // lazily, inside its own profiling scope
    if (!g->dinv_ev && hipEventCreateWithFlags(&g->dinv_ev, hipEventDisableTiming) != hipSuccess) return;   // (a set member's first use; without the event: built lazily by the next prediction)
    if (gate_value) {
        hipLaunchKernelGGL(potrf_gate_kernel, dim3(1), dim3(64), 0, c->side_stream, c->sig_panel, gate_value, g->info, poll_budget_ticks(g->Np));
    } else {
        (void)hipEventRecord(c->ev_fork, c->stream);
        (void)hipStreamWaitEvent(c->side_stream, c->ev_fork, 0);
    }
    dinv_launch(g, c->side_stream);
    if (g->W2 && g->w2_np == g->Np && g->w2_used) {          // the few-candidates steps of the last factorisation used W: build it here too
        hipLaunchKernelGGL(few_w_kernel<PredG32>, dim3(PRED_RB / 32, 2 * (g->Np / PRED_RB)), dim3(PredG32::NTHREADS), PredictLds<PredG32>::BYTES,
                           c->side_stream, (const double*)g->A, g->ld, (const double*)g->Dinv2, g->W2);
        g->w2_gen = g->factor_gen;
    }
    g->w2_used = false;
    (void)hipEventRecord(g->dinv_ev, c->side_stream);
    g->dinv_pending = true;
    g->have_dinv = true;
}

// the side stream may still be reading A / inv16 for the previous factorisation's inverses
static void dinv_join(boss_gp* g) {
    if (g->dinv_pending) {
        (void)hipStreamWaitEvent(g->ctx->stream, g->dinv_ev, 0);
        g->dinv_pending = false;
    }
}

// Gram + blocked Cholesky + solves + logdet of the handle's resident data under its resident
// hyper-parameters; results land in host_res when the stream drains.
static int factor_enqueue(boss_gp* g, RiderReq* rider) {
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    static const bool watch = getenv("BOSS_DEBUG_WATCH") && atoi(getenv("BOSS_DEBUG_WATCH"));
    struct Note { bool on; ~Note() { if (on) std::fprintf(stderr, "[bosship watch] factor_enqueue done\n"); } } note_{watch};
    if (watch) std::fprintf(stderr, "[bosship watch] factor_enqueue Np %d\n", g->Np);
    dinv_join(g);
    ++g->factor_gen;                                         // whatever was derived from the old factor on its own (block 0 of Dinv) is stale
    if (launch_stamps_on()) g_stamps.reset();
    BOSS_STAMP(1);
    const ChainPlan plan = chain_begin(c, g->A, g->ld, g->Np, g->inv16, g->info);
    BOSS_STAMP(2);
    // (the resident strips recognise an inverse tile the chain has not written yet by this pattern: follow_strip, chain.hpp)
    const bool fill_in_prep = plan.on && !g->aug && !g->gibbs && !g->kprog && g->par_in_args;   // (scale_points_args_kernel writes the pattern itself)
    if (plan.on && !fill_in_prep) (void)hipMemsetAsync(g->inv16, 0xff, sizeof(double) * (size_t)g->nblk * 8 * 256, s);
    {
        ProfScope ps(c, "prep");
        bool rhs_done = false;
        if (!g->aug && !g->gibbs) {
            if (g->par_in_args) {
                HypArgs par;
                par.d = g->d;
                for (int k = 0; k < g->d; ++k) par.invlam[k] = g->host_par[k];
                par.hyp[0] = g->host_par[g->d];
                par.hyp[1] = g->host_par[g->d + 1];
                hipLaunchKernelGGL(scale_points_args_kernel, dim3((g->Np + 255) / 256, 1, 1), dim3(256), 0, s, par,
                                   (const double*)g->Xraw, g->Xsc, g->invlam, g->Np, g->A, g->ld, g->N, (const double*)g->y,
                                   (const double*)g->mean, g->info, fill_in_prep ? g->inv16 : (double*)nullptr);   // scaled points, δ^T rows, cleared failed-pivot flag
                rhs_done = true;
            } else {
                hipLaunchKernelGGL(scale_points_kernel, dim3((g->Np + 255) / 256, 1, 1), dim3(256), 0, s, g->Xraw, g->Xsc,
                                   (size_t)0, g->invlam, g->d, g->Np);
            }
        }
        if (!rhs_done)
            hipLaunchKernelGGL(rhs_rows_kernel, dim3((g->Np + 255) / 256, 1, 1), dim3(256), 0, s, g->A, g->ld, (size_t)0,
                               g->N, g->Np, g->y, g->mean, (size_t)0, 0, g->info);   // also clears the failed-pivot flag
    }
    if (g->aug) {
        ProfScope ps(c, "gram");
        const long long t64 = g->Np / 64;
        hipLaunchKernelGGL(aug_gram_kernel, dim3((unsigned)(t64 * (t64 + 1) / 2)), dim3(256), 0, s, (const double*)g->Xraw, g->ldx,
                           g->d, g->nhead, g->N, g->Np, g->kernel, (const double*)g->hyp, (const double*)g->invlam, (size_t)0, g->A,
                           g->ld, (size_t)0, 0);
    } else if (g->gibbs) {
        ProfScope ps(c, "gram");
        const int t64 = g->Np / 64;
        hipLaunchKernelGGL(gibbs_gram_kernel, dim3(t64 * (t64 + 1) / 2), dim3(256), 0, s, (const double*)g->Xraw,
                           (const double*)g->lamX, (const double*)g->ampX, (const double*)g->noiseX, (size_t)0, (size_t)0, g->d, g->N,
                           g->Np, g->A, g->ld, (size_t)0, 0);
    } else if (g->kprog) {
        ProfScope ps(c, "gram");
        kprog_gram_launch(g, s);
    } else {
        gram_enqueue(c, g->Xsc, 0, g->d, g->N, g->Np, g->kernel, g->hyp, g->A, g->ld, 0, 1);
    }
    BOSS_STAMP(3);
    chain_ready(c, plan, g->Np, g->info);
    const bool riding = rider && plan.on && rider->step && chain_trail_mode(g->nblk) != 2 && g->par_in_args && !g->kprog;
    if (rider) rider->plan = riding ? plan : ChainPlan();
    potrf_enqueue(c, g->A, g->ld, g->Np, 1, 0, g->inv16, 0, g->info, true, &plan, riding ? &rider->step : nullptr);
    // the block inverses go on the side stream right away only when the previous factorisation's were used (update → predict
    // patterns); likelihood-only loops (fitters) never pay for them, a first prediction builds them itself
    g->gated = c->sig_panel != nullptr;                      // this update may contain gate kernels (gp_finish: fallback on their timeout)
    g->chained = plan.on;                                    // ... and ran under the resident chain
    const int trail = chain_trail_mode(g->nblk);             // (mode 4 without its work table runs the per-step launches of mode 0)
    g->trail_used = !plan.on ? -1 : trail == 4 ? (plan.tab ? 4 : 0) : (trail == 1 || trail == 2) ? trail : 0;
    // (with a rider the side stream is busy with the candidates' substitution, which needs no block inverses: a later prediction
    // builds them itself)
    const bool eager = g->dinv_used && !c->prof_on && !rider;
    const unsigned long long pending = ((eager || rider) && c->sig_panel) ? ++c->sig_seq : 0;   // the log-det kernel's entry releases them
    if (rider) rider->end_gate = pending;
    g->dinv_used_prev = g->dinv_used;
    g->dinv_used = false;
    {
        // logdet, zᵀz and info land in mapped host memory straight from the kernel (no copy behind it)
        ProfScope ps(c, "logdet");
        hipLaunchKernelGGL(potrf_logdet_kernel, dim3(1, 1, 1), dim3(LOGDET_THREADS), 0, s, g->A, g->ld, (size_t)0, g->N, g->Np,
                           g->scal, g->host_res_dev, (const int*)g->info, pending ? c->sig_panel : (unsigned long long*)nullptr, pending,
                           ++g->res_seq);
    }
    g->res_polled = true;
    BOSS_STAMP(4);
    if (eager) dinv_eager(g, pending);
    BOSS_STAMP(5);
    return BOSS_OK;
}

// Everything of boss_gp_update up to the wait: parameters staged, the update enqueued (caller holds the context's lock).
// rider (or null): a candidate batch wants to ride along — filled in when the update runs under the resident chain (plan.on).
static int gp_update_enqueue(boss_gp* g, const double* lengthscale, double amplitude, double noise_std, const double* mean_X,
                             RiderReq* rider) {
    Ctx* c = g->ctx;
    hipStream_t s = c->stream;
    gp_invalidate(g);
    const bool small = small_fit_ok(c, g->N, g->d) && !g->kprog;   // one launch does it all (built-in kernels only)
    if (!g->par_ev) {                         // a member of a batch-fitted set: created here, on its first update (boss_gp_fit_batch)
        HIPCHK(hipEventCreateWithFlags(&g->par_ev, hipEventDisableTiming));
        if (!g->dinv_ev) HIPCHK(hipEventCreateWithFlags(&g->dinv_ev, hipEventDisableTiming));
    }
    HIPCHK(hipEventSynchronize(g->par_ev));   // previous update's staging copies have been consumed
    double* invlam = g->host_par;
    double* hyp = g->host_par + g->d;
    (void)stage_hyper(g->d, lengthscale, amplitude, noise_std, invlam, hyp);   // (validated by the caller)
    g->amp2 = hyp[0];
    g->par_in_args = !small && g->d <= HYP_ARGS_MAX_D && !g->kprog;          // the first kernel of the update deposits them on the device
    if (!small && !g->par_in_args) {
        HIPCHK(hipMemcpyAsync(g->invlam, invlam, sizeof(double) * (g->d + 2), hipMemcpyHostToDevice, s));   // hyp follows invlam on both sides
        HIPCHK(hipEventRecord(g->par_ev, s));
    }
    if (mean_X) {
        HIPCHK(hipMemcpyAsync(g->mean, mean_X, sizeof(double) * g->N, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));      // caller's (pageable) mean buffer may be reused on return
        g->has_mean = true;
    } else if (g->has_mean) {
        HIPCHK(hipMemsetAsync(g->mean, 0, sizeof(double) * g->Np, s));
        g->has_mean = false;
    }
    if (small) {
        // N <= 128: scaled points, Gram, factorisation, z, logdet in ONE launch; the hyper-parameters travel in the kernel
        // arguments and the results land in mapped host memory (no copies)
        dinv_join(g);
        ++g->factor_gen;
        SmallFitPar par;
        par.d = g->d;
        par.N = g->N;
        par.Np = g->Np;
        par.ld = g->ld;
        par.kern = g->kernel;
        par.amp2 = hyp[0];
        par.sig2 = hyp[1];
        for (int k = 0; k < g->d; ++k) par.invlam[k] = invlam[k];
        hipLaunchKernelGGL(small_fit_kernel, dim3(1), dim3(DIAG_THREADS), SMALL_LDS_BYTES, s, par, (const double*)g->Xraw, g->Xsc,
                           (const double*)g->y, (const double*)g->mean, g->A, g->inv16, g->invlam, g->scal, g->info, g->host_res_dev,
                           ++g->res_seq);
        g->res_polled = true;
        g->chained = false;
        g->trail_used = -1;
        if (g->dinv_used) dinv_eager(g);
        g->dinv_used = false;
    } else {
        int rc = factor_enqueue(g, rider);
        if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    g->pending = true;
    return BOSS_OK;
}

extern "C" int boss_gp_update(boss_gp_t* g, const double* lengthscale, double amplitude, double noise_std,
                              const double* mean_X, int flags, double* logpdf_out) {
    if (!g) return fail(BOSS_E_INVALID, "gp is NULL");
    NOT_FOR_MODELS(g);                                       // (program-kernel posteriors update here too)
    int rc = validate_hyper(g->d, lengthscale, amplitude, noise_std);
    if (rc) return rc;
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);                 // streams, events and scratch of the device context are shared
    rc = gp_update_enqueue(g, lengthscale, amplitude, noise_std, mean_X, nullptr);
    if (rc) return rc;
    if (flags & BOSS_FIT_NO_SYNC) return BOSS_OK;
    return gp_finish(g, logpdf_out);
}

// model_posterior_slice / data_loglike of GradientGaussianProcess (gradient_gp.jl:307-329, :367-397):
// augmented Gram, Cholesky, α-solve and log marginal likelihood under (λ, α, σ, σ_∂).
extern "C" int boss_ggp_update(boss_gp_t* g, const double* lengthscale, double amplitude, double noise_std,
                               double grad_noise_std, int flags, double* logpdf_out) {
    if (!g) return fail(BOSS_E_INVALID, "gp is NULL");
    if (!g->aug) return fail(BOSS_E_INVALID, "handle was not created by boss_ggp_create");
    int rc = validate_hyper(g->d, lengthscale, amplitude, noise_std);
    if (rc) return rc;
    if (!(grad_noise_std >= 0.0)) return fail(BOSS_E_INVALID, "grad_noise_std must be >= 0");
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    gp_invalidate(g);
    if (!g->par_ev) HIPCHK(hipEventCreateWithFlags(&g->par_ev, hipEventDisableTiming));   // (a member of a batch-fitted set: its first update)
    HIPCHK(hipEventSynchronize(g->par_ev));
    double* invlam = g->host_par;
    double* hyp = g->host_par + g->d;
    (void)stage_hyper(g->d, lengthscale, amplitude, noise_std, invlam, hyp);   // gradient_gp.jl:128-131, :200-204 (validated above)
    const double sgd = grad_noise_std + MIN_PARAM_VALUE;
    hyp[2] = sgd * sgd;
    g->amp2 = hyp[0];
    HIPCHK(hipMemcpyAsync(g->invlam, invlam, sizeof(double) * (g->d + 3), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(g->par_ev, s));
    rc = factor_enqueue(g);
    if (rc) return rc;
    return update_finish(g, flags, logpdf_out);
}

// finite_nongp + logpdf / posterior (nonstationary_gp.jl:153-196, :237-245): the caller evaluates its latent
// models at the training points — lam_X d×N (column j = λ(x_j)), amp_X N, noise_X N.
extern "C" int boss_ngp_update(boss_gp_t* g, const double* lam_X, const double* amp_X, const double* noise_X,
                               const double* mean_X, int flags, double* logpdf_out) {
    if (!g || !lam_X || !amp_X || !noise_X) return fail(BOSS_E_INVALID, "NULL argument");
    if (!g->gibbs) return fail(BOSS_E_INVALID, "handle was not created by boss_ngp_create");
    const int d = g->d, N = g->N, Np = g->Np;
    std::vector<double> lam((size_t)d * Np, 1.0), amp(Np, 0.0), noi(Np, 0.0);
    for (int j = 0; j < N; ++j) {
        for (int k = 0; k < d; ++k) {
            const double v = lam_X[(size_t)j * d + k];
            if (!(v > 0.0) || !std::isfinite(v)) return fail(BOSS_E_INVALID, "lengthscales must be finite and > 0");
            lam[(size_t)k * Np + j] = v;
        }
        if (!(amp_X[j] >= 0.0) || !std::isfinite(amp_X[j])) return fail(BOSS_E_INVALID, "amplitudes must be finite and >= 0");
        if (!(noise_X[j] >= 0.0) || !std::isfinite(noise_X[j])) return fail(BOSS_E_INVALID, "noise stds must be finite and >= 0");
        amp[j] = amp_X[j];
        noi[j] = noise_X[j];
    }
    Ctx* c = g->ctx;
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> lk(c->mtx);
    hipStream_t s = c->stream;
    gp_invalidate(g);
    HIPCHK(hipMemcpyAsync(g->lamX, lam.data(), sizeof(double) * d * Np, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->ampX, amp.data(), sizeof(double) * Np, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->noiseX, noi.data(), sizeof(double) * Np, hipMemcpyHostToDevice, s));
    if (mean_X) {
        HIPCHK(hipMemcpyAsync(g->mean, mean_X, sizeof(double) * N, hipMemcpyHostToDevice, s));
        g->has_mean = true;
    } else if (g->has_mean) {
        HIPCHK(hipMemsetAsync(g->mean, 0, sizeof(double) * Np, s));
        g->has_mean = false;
    }
    HIPCHK(hipStreamSynchronize(s));                         // the staging vectors go out of scope
    int rc = factor_enqueue(g);
    if (rc) return rc;
    return update_finish(g, flags, logpdf_out);
}

extern "C" int boss_gp_sync(boss_gp_t* g, double* logpdf_out) {
    if (!g) return fail(BOSS_E_INVALID, "gp is NULL");
    HIPCHK(hipSetDevice(g->ctx->device));
    std::lock_guard<std::mutex> lk(g->ctx->mtx);
    if (!g->pending) {
        if (!g->fitted) return fail(BOSS_E_NOT_FITTED, "no update pending and handle is not fitted");
        if (logpdf_out) *logpdf_out = loglik(g->N, g->host_res[0], g->host_res[1]);
        return BOSS_OK;
    }
    return gp_finish(g, logpdf_out);
}
