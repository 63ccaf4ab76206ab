// host_multi.inc — ONE process driving G devices: the shard modes of SURVEY §8e behind the C ABI (included by bosship.hip).
//
// What a Julia caller (no torch, no MPI) needs to spread the acquisition path over the GPUs of a node:
//   boss_init                 enumerate the devices, one context each, one RCCL communicator per device (ncclCommInitAll)
//   boss_multi_gp_update      the same hyper-parameters on G replicas of a posterior, all devices factorising concurrently
//   boss_multi_acq_ei         candidates sharded M/G over replicated posteriors; ONE 16-byte-per-rank RCCL all-gather
//                             of (max, global index), reduced identically for every device            (config 3)
//   boss_multi_acq_ei_outputs output p lives on ONE device; its (mu, var) rows travel in ONE RCCL all-reduce(sum) over
//                             zero-filled rows (exact), then the EI x feasibility epilogue + arg-max   (config 4)
//   boss_multi_acq_ei_samples hyper-parameter sample s lives on ONE device; per-device partial sums of acq_s(x_j),
//                             ONE RCCL all-reduce(sum) of M doubles, /S, mask, arg-max                 (config 5)
//   boss_multi_loglike_batch  S hyper-parameter sets split over the devices, no collective
// The devices work concurrently (one host thread per device inside the call).  RCCL is loaded at run time
// (dlopen librccl.so.1): the single-device library has no hard dependency on it, a multi-device call without it fails loudly.
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <condition_variable>
#include <thread>

struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

struct Multi {
    bool inited = false, rccl = false;
    bool host_exchange = false;                 // BOSS_VIRTUAL_DEVICES: reductions and gathers through host memory
    int G = 0;
    RcclApi api;
    std::vector<Ctx*> ctx;
    std::vector<ncclComm_t> comm;
    std::vector<double*> xsend, xrecv;          // per device: 2 doubles out, 2·G doubles in (the arg-max exchange)
    std::vector<Workspace> red;                 // per device: operand of the larger all-reduces
    std::string why_no_rccl;
};
static Multi g_multi;
static std::mutex g_multi_mtx;
static void workers_stop();

static bool rccl_load(RcclApi& a, std::string& why) {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        a.h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (a.h) break;
    }
    if (!a.h) {
        why = std::string("librccl.so.1 could not be loaded: ") + (dlerror() ? dlerror() : "?");
        return false;
    }
    a.CommInitAll = (decltype(a.CommInitAll))dlsym(a.h, "ncclCommInitAll");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(a.h, "ncclCommDestroy");
    a.AllGather = (decltype(a.AllGather))dlsym(a.h, "ncclAllGather");
    a.AllReduce = (decltype(a.AllReduce))dlsym(a.h, "ncclAllReduce");
    a.GroupStart = (decltype(a.GroupStart))dlsym(a.h, "ncclGroupStart");
    a.GroupEnd = (decltype(a.GroupEnd))dlsym(a.h, "ncclGroupEnd");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(a.h, "ncclGetErrorString");
    if (!a.CommInitAll || !a.CommDestroy || !a.AllGather || !a.AllReduce || !a.GroupStart || !a.GroupEnd || !a.GetErrorString) {
        why = "librccl.so.1 lacks an expected symbol";
        return false;
    }
    return true;
}

extern "C" int boss_init(int* n_devices_out) {
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    Multi& m = g_multi;
    if (m.inited) {
        if (n_devices_out) *n_devices_out = m.G;
        return BOSS_OK;
    }
    int n = visible_devices();
    if (n <= 0) {
        if (n_devices_out) *n_devices_out = 0;
        return fail(BOSS_E_NO_DEVICE, "no HIP device visible (bosship has no CPU fallback)");
    }
    if (const char* lim = getenv("BOSS_MAX_DEVICES")) n = std::max(1, std::min(n, atoi(lim)));
    m.ctx.assign(n, nullptr);
    for (int g = 0; g < n; ++g) {
        int rc = get_ctx(g, &m.ctx[g]);
        if (rc) return rc;
    }
    m.G = n;
    m.rccl = false;
    m.host_exchange = virtual_devices() > 0;                 // several contexts on one physical device: no communicator possible
    if (m.host_exchange) m.why_no_rccl = "BOSS_VIRTUAL_DEVICES: exchanges go through the host";
    else if (rccl_load(m.api, m.why_no_rccl)) {
        std::vector<int> devs(n);
        for (int g = 0; g < n; ++g) devs[g] = g;
        m.comm.assign(n, nullptr);
        ncclResult_t r = m.api.CommInitAll(m.comm.data(), n, devs.data());
        if (r == ncclSuccess) m.rccl = true;
        else m.why_no_rccl = std::string("ncclCommInitAll: ") + m.api.GetErrorString(r);
    }
    if (!m.rccl && n > 1 && !m.host_exchange) {
        m.G = 0;
        return fail(BOSS_E_NO_DEVICE, "multi-device needs RCCL: " + m.why_no_rccl);
    }
    m.xsend.assign(n, nullptr);
    m.xrecv.assign(n, nullptr);
    m.red.assign(n, Workspace());
    for (int g = 0; g < n; ++g) {
        HIPCHK(hipSetDevice(m.ctx[g]->device));
        if (dev_malloc((void**)&m.xsend[g], sizeof(double) * 2) != hipSuccess ||
            dev_malloc((void**)&m.xrecv[g], sizeof(double) * 2 * n) != hipSuccess)
            return fail(BOSS_E_ALLOC, "device allocation failed");
    }
    m.inited = true;
    if (n_devices_out) *n_devices_out = n;
    return BOSS_OK;
}

extern "C" int boss_comm_info(int* n_devices_out, int* rccl_out) {
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    if (n_devices_out) *n_devices_out = g_multi.inited ? g_multi.G : 0;
    if (rccl_out) *rccl_out = g_multi.inited && g_multi.rccl ? 1 : 0;
    return g_multi.inited ? BOSS_OK : fail(BOSS_E_INVALID, "boss_init has not been called");
}

extern "C" void boss_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    Multi& m = g_multi;
    if (!m.inited) return;
    for (int g = 0; g < m.G; ++g) {
        (void)hipSetDevice(m.ctx[g]->device);
        (void)hipStreamSynchronize(m.ctx[g]->stream);
        if (m.rccl && m.comm[g]) (void)m.api.CommDestroy(m.comm[g]);
        if (m.xsend[g]) (void)hipFree(m.xsend[g]);
        if (m.xrecv[g]) (void)hipFree(m.xrecv[g]);
        if (m.red[g].p) (void)hipFree(m.red[g].p);
    }
    m.comm.clear();
    m.xsend.clear();
    m.xrecv.clear();
    m.red.clear();
    m.ctx.clear();
    workers_stop();
    m.inited = false;
    m.rccl = false;
    m.G = 0;                                                 // the RCCL library itself stays loaded
}

static int multi_ready(int G) {
    if (!g_multi.inited) return fail(BOSS_E_INVALID, "call boss_init first");
    if (G < 1 || G > g_multi.G) return fail(BOSS_E_INVALID, "device count outside 1..boss_init's count");
    return BOSS_OK;
}

#define RCCLCHK(expr)                                                                                           \
    do {                                                                                                        \
        ncclResult_t r_ = (expr);                                                                               \
        if (r_ != ncclSuccess) return fail(BOSS_E_NO_DEVICE, std::string(#expr) + ": " + g_multi.api.GetErrorString(r_)); \
    } while (0)

// contiguous balanced shard [lo, hi) of n items over G parts (first n % G parts get one extra) — get_sample_counts
// (src/utils/sampling.jl:6-13) as ranges
static inline void shard_range(long n, int g, int G, long* lo, long* hi) {
    const long base = n / G, rem = n % G;
    *lo = g * base + std::min<long>(g, rem);
    *hi = *lo + base + (g < rem ? 1 : 0);
}

// larger value wins, NaN counts as the largest (Julia argmax), ties go to the smaller index
static inline bool pair_better(double a, long ia, double b, long ib) {
    const bool an = a != a, bn = b != b;
    if (an != bn) return an;
    if (!an && a != b) return a > b;
    return ia < ib;
}

// One resident worker thread per device beyond the first (started by boss_init, ended by boss_shutdown): a multi-device call hands
// every device its share and the calling thread takes device 0's.  (A std::thread per device per call cost 30-60 µs of a
// 0.2-2 ms call.)
struct DevWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool busy = false, quit = false;
    void loop() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return quit || (bool)job; });
            if (quit) return;
            std::function<void()> j = std::move(job);
            job = nullptr;
            lk.unlock();
            j();
            lk.lock();
            busy = false;
            cv.notify_all();
        }
    }
    void submit(std::function<void()> j) {
        std::unique_lock<std::mutex> lk(mu);
        job = std::move(j);
        busy = true;
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !busy; });
    }
};
static std::vector<DevWorker*> g_workers;                    // [g - 1] serves device g
static void workers_start(int G) {
    for (int g = (int)g_workers.size() + 1; g < G; ++g) {
        DevWorker* w = new DevWorker();
        w->th = std::thread([w] { w->loop(); });
        g_workers.push_back(w);
    }
}
static void workers_stop() {
    for (DevWorker* w : g_workers) {
        {
            std::unique_lock<std::mutex> lk(w->mu);
            w->quit = true;
            w->cv.notify_all();
        }
        w->th.join();
        delete w;
    }
    g_workers.clear();
}

// run fn(g) for g = 0..G-1, device g > 0 on its worker thread; first failing status (and its message) wins
template <class F>
static int on_devices(int G, F fn) {
    std::vector<int> rc(G, BOSS_OK);
    std::vector<std::string> msg(G);
    workers_start(G);
    for (int g = 1; g < G; ++g)
        g_workers[g - 1]->submit([&, g]() {
            rc[g] = fn(g);
            if (rc[g]) msg[g] = g_last_error;                // thread-local: carry it out
        });
    rc[0] = fn(0);
    if (rc[0]) msg[0] = g_last_error;
    for (int g = 1; g < G; ++g) g_workers[g - 1]->wait();
    for (int g = 0; g < G; ++g)
        if (rc[g]) return fail(rc[g], msg[g]);
    return BOSS_OK;
}

extern "C" int boss_multi_gp_update(int G, boss_gp_t* const* gps, const double* lengthscale, double amplitude, double noise_std,
                                    const double* mean_X, double* logpdf_out) {
    if (!gps || G < 1) return fail(BOSS_E_INVALID, "bad arguments");
    for (int g = 0; g < G; ++g) {
        if (!gps[g]) return fail(BOSS_E_INVALID, "NULL posterior handle");
        NOT_FOR_KPROG(gps[g]);
    }
    int first = BOSS_OK;
    std::string msg;
    for (int g = 0; g < G; ++g) {                            // enqueue everywhere, then wait: the devices factorise concurrently
        int rc = boss_gp_update(gps[g], lengthscale, amplitude, noise_std, mean_X, BOSS_FIT_NO_SYNC, nullptr);
        if (rc && !first) {
            first = rc;
            msg = g_last_error;
        }
    }
    for (int g = 0; g < G; ++g) {
        double lp = 0.0;
        int rc = gps[g]->pending ? boss_gp_sync(gps[g], &lp) : BOSS_OK;
        if (rc && !first) {
            first = rc;
            msg = g_last_error;
        }
        if (g == 0 && logpdf_out) *logpdf_out = rc ? -std::numeric_limits<double>::infinity() : lp;
    }
    return first ? fail(first, msg) : BOSS_OK;
}

// Candidates resident on G devices: shard g = columns [lo_g, hi_g) of Xs on device g (boss_multi_cand_create).  A maximiser that
// evaluates the same candidates for several acquisition calls (a BO iteration's P×S posteriors, a sequential batch) uploads once.
struct boss_multi_cand {
    int G = 0, d = 0, M = 0;
    std::vector<boss_cand_t*> shard;                         // null where the shard is empty
    std::vector<long> lo;
};

static void multi_cand_release(boss_multi_cand* mc) {
    if (!mc) return;
    for (boss_cand_t* c : mc->shard)
        if (c) boss_cand_free(c);
    delete mc;
}

static int multi_cand_build(int G, int d, int M, const double* Xs, boss_multi_cand** out) {
    boss_multi_cand* mc = new boss_multi_cand();
    mc->G = G;
    mc->d = d;
    mc->M = M;
    mc->shard.assign(G, nullptr);
    mc->lo.assign(G + 1, 0);
    for (int g = 0; g < G; ++g) {
        long lo, hi;
        shard_range(M, g, G, &lo, &hi);
        mc->lo[g] = lo;
        mc->lo[g + 1] = hi;
    }
    int rc = on_devices(G, [&](int g) -> int {
        const long n = mc->lo[g + 1] - mc->lo[g];
        return n > 0 ? boss_cand_create(g_multi.ctx[g]->logical, d, (int)n, Xs + (size_t)d * mc->lo[g], &mc->shard[g]) : BOSS_OK;
    });
    if (rc) {
        std::string keep = g_last_error;
        multi_cand_release(mc);
        return fail(rc, keep);
    }
    *out = mc;
    return BOSS_OK;
}

extern "C" int boss_multi_cand_create(int G, int d, int M, const double* Xs, boss_multi_cand_t** out) {
    if (!out) return fail(BOSS_E_INVALID, "out is NULL");
    *out = nullptr;
    if (d < 1 || M < 1 || !Xs) return fail(BOSS_E_INVALID, "need d >= 1, M >= 1 and non-NULL Xs");
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    int rc = multi_ready(G);
    if (rc) return rc;
    return multi_cand_build(G, d, M, Xs, out);
}

extern "C" void boss_multi_cand_free(boss_multi_cand_t* mc) { multi_cand_release(mc); }

// The sharded acquisition on resident candidates.  Per device: prediction + EI epilogue enqueued without waiting, the epilogue
// leaves (max, GLOBAL index) in the device's 16-byte send buffer, the all-gather follows on the same stream, ONE download of the
// 2·G doubles and one wait per device.  (The call holds the library's multi-device lock: collectives of one communicator must be
// issued in one order.)
static int multi_acq_ei_on(Multi& m, int G, int P, int S, boss_gp_t* const* gps, const boss_multi_cand* mc, const double* mean_Xs,
                           const double* fit_coefs, const double* y_max, int has_best, double best, const unsigned char* valid_mask,
                           double* acq_out, long* argmax_out, double* max_out) {
    const size_t PS = (size_t)P * S;
    const int M = mc->M;
    for (int g = 0; g < G; ++g)
        for (size_t i = 0; i < PS; ++i) {
            const boss_gp* h = gps[PS * g + i];
            if (!h) return fail(BOSS_E_INVALID, "NULL posterior handle");
            NOT_FOR_KPROG(h);
            if (h->ctx != m.ctx[g]) return fail(BOSS_E_INVALID, "replica g of every posterior must live on device g");
            if (h->d != mc->d) return fail(BOSS_E_INVALID, "candidates and posteriors differ in x_dim");
        }
    const bool collective = m.rccl && G == m.G && G > 1;
    std::vector<char> has(G, 0);
    int rc = on_devices(G, [&](int g) -> int {
        const long lo = mc->lo[g], hi = mc->lo[g + 1];
        const int Mg = (int)(hi - lo);
        HIPCHK(hipSetDevice(m.ctx[g]->device));
        if (Mg == 0) {
            // an empty shard still takes part in the collective: (-Inf, M) loses against every real pair
            const double none[2] = {-std::numeric_limits<double>::infinity(), (double)M};
            if (collective) HIPCHK(hipMemcpyAsync(m.xsend[g], none, sizeof none, hipMemcpyHostToDevice, m.ctx[g]->stream));
            if (collective) HIPCHK(hipStreamSynchronize(m.ctx[g]->stream));
            return BOSS_OK;
        }
        std::vector<double> msh;
        if (mean_Xs) {                                       // p + P*(j + M*s)  ->  p + P*((j - lo) + Mg*s)
            msh.resize((size_t)P * Mg * S);
            for (int s = 0; s < S; ++s)
                std::memcpy(&msh[(size_t)P * Mg * s], mean_Xs + (size_t)P * (lo + (size_t)M * s), sizeof(double) * P * Mg);
        }
        has[g] = 1;
        int r = acq_ei_impl(P, S, gps + PS * g, mc->shard[g], mean_Xs ? msh.data() : nullptr, fit_coefs, y_max, has_best, best,
                            valid_mask ? valid_mask + lo : nullptr, acq_out ? acq_out + lo : nullptr, nullptr, nullptr, m.xsend[g], lo,
                            /*defer=*/true);
        // (msh, and the caller's mask / acq_out ranges, are read or written by copies still in flight: wait here unless the
        // collective below is going to wait anyway — the copies of this call precede it on the stream)
        if (r || !collective || mean_Xs) (void)hipStreamSynchronize(m.ctx[g]->stream);
        return r;
    });
    if (rc) {
        for (int g = 0; g < G; ++g) {
            (void)hipSetDevice(m.ctx[g]->device);
            (void)hipStreamSynchronize(m.ctx[g]->stream);
        }
        return rc;
    }
    double bv = -std::numeric_limits<double>::infinity();
    long bi = (long)M;
    if (collective) {
        std::vector<double> all(2 * (size_t)G);
        RCCLCHK(m.api.GroupStart());
        for (int g = 0; g < G; ++g)
            RCCLCHK(m.api.AllGather(m.xsend[g], m.xrecv[g], 2, ncclDouble, m.comm[g], m.ctx[g]->stream));
        RCCLCHK(m.api.GroupEnd());
        HIPCHK(hipSetDevice(m.ctx[0]->device));
        HIPCHK(hipMemcpyAsync(all.data(), m.xrecv[0], sizeof(double) * 2 * G, hipMemcpyDeviceToHost, m.ctx[0]->stream));
        for (int g = 0; g < G; ++g) {
            HIPCHK(hipSetDevice(m.ctx[g]->device));
            HIPCHK(hipStreamSynchronize(m.ctx[g]->stream));
        }
        for (int g = 0; g < G; ++g)
            if (pair_better(all[2 * g], (long)all[2 * g + 1], bv, bi)) {
                bv = all[2 * g];
                bi = (long)all[2 * g + 1];
            }
    } else {
        // one device, a subset of the communicator's devices, or virtual devices: every shard's pair is in its context's pinned block
        for (int g = 0; g < G; ++g) {
            if (!has[g]) continue;
            const double* hres = (const double*)m.ctx[g]->pinned + MULTI_RES_OFF;   // (the deferred shard's own area: acq_ei_impl)
            long li;
            std::memcpy(&li, &hres[1], sizeof(long));
            if (pair_better(hres[0], li + mc->lo[g], bv, bi)) {
                bv = hres[0];
                bi = li + mc->lo[g];
            }
        }
    }
    if (argmax_out) *argmax_out = bi;
    if (max_out) *max_out = bv;
    return BOSS_OK;
}

extern "C" int boss_multi_acq_ei_cand(int G, int P, int S, boss_gp_t* const* gps, const boss_multi_cand_t* cand, const double* mean_Xs,
                                      const double* fit_coefs, const double* y_max, int has_best, double best,
                                      const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    if (P < 1 || S < 1 || !gps || !cand || !fit_coefs) return fail(BOSS_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    int rc = multi_ready(G);
    if (rc) return rc;
    if (cand->G != G) return fail(BOSS_E_INVALID, "the candidates were sharded over a different number of devices");
    return multi_acq_ei_on(g_multi, G, P, S, gps, cand, mean_Xs, fit_coefs, y_max, has_best, best, valid_mask, acq_out, argmax_out, max_out);
}

extern "C" int boss_multi_acq_ei(int G, int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                 const double* fit_coefs, const double* y_max, int has_best, double best,
                                 const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    if (P < 1 || S < 1 || M < 1 || !gps || !Xs || !fit_coefs) return fail(BOSS_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    int rc = multi_ready(G);
    if (rc) return rc;
    if (!gps[0]) return fail(BOSS_E_INVALID, "NULL posterior handle");
    boss_multi_cand* mc = nullptr;
    rc = multi_cand_build(G, gps[0]->d, M, Xs, &mc);          // one-shot shards (resident ones: boss_multi_cand_create + boss_multi_acq_ei_cand)
    if (rc) return rc;
    rc = multi_acq_ei_on(g_multi, G, P, S, gps, mc, mean_Xs, fit_coefs, y_max, has_best, best, valid_mask, acq_out, argmax_out, max_out);
    std::string keep = g_last_error;
    multi_cand_release(mc);
    g_last_error = keep;
    return rc;
}

// in-place all-reduce(sum) of `count` doubles held in m.red[g] on every device of the communicator
static int multi_allreduce(Multi& m, size_t count) {
    if (!m.rccl && m.host_exchange && m.G > 1) {
        // virtual devices: the same sum through host memory, in device order (x + 0 + ... stays exact for the moment blocks)
        std::vector<double> acc(count, 0.0), tmp(count);
        for (int g = 0; g < m.G; ++g) {
            HIPCHK(hipSetDevice(m.ctx[g]->device));
            HIPCHK(hipMemcpyAsync(tmp.data(), m.red[g].p, sizeof(double) * count, hipMemcpyDeviceToHost, m.ctx[g]->stream));
            HIPCHK(hipStreamSynchronize(m.ctx[g]->stream));
            for (size_t i = 0; i < count; ++i) acc[i] += tmp[i];
        }
        for (int g = 0; g < m.G; ++g) {
            HIPCHK(hipSetDevice(m.ctx[g]->device));
            HIPCHK(hipMemcpyAsync(m.red[g].p, acc.data(), sizeof(double) * count, hipMemcpyHostToDevice, m.ctx[g]->stream));
            HIPCHK(hipStreamSynchronize(m.ctx[g]->stream));
        }
        return BOSS_OK;
    }
    if (!m.rccl) return BOSS_OK;                             // one device without RCCL: the sum is the operand
    RCCLCHK(m.api.GroupStart());
    for (int g = 0; g < m.G; ++g)
        RCCLCHK(m.api.AllReduce(m.red[g].p, m.red[g].p, count, ncclDouble, ncclSum, m.comm[g], m.ctx[g]->stream));
    RCCLCHK(m.api.GroupEnd());
    return BOSS_OK;
}

// EI x feasibility epilogue + arg-max on `c` from moments resident on that device (mu/var: [S][P][M]); the acquisition
// values land in dacq (device, M doubles)
static int moments_epilogue_dev(Ctx* c, int P, int S, int M, const double* dmu, const double* dvar, double* dacq,
                                const double* fit_coefs, const double* y_max, int has_best, double best,
                                const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    hipStream_t s = c->stream;
    int rc = ws_reserve(c->acq, sizeof(double) * (2 * (size_t)P) + M + 64);
    if (rc) return rc;
    double* dcoef = (double*)c->acq.p;
    double* dymax = dcoef + P;
    unsigned char* dmask = (unsigned char*)(dymax + P);
    double* hres = (double*)c->pinned;
    EiPar par;
    rc = ei_params(c, s, P, fit_coefs, y_max, has_best, best, &par, dcoef, dymax);
    if (rc) return rc;
    const size_t pm = (size_t)P * M;
    if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
    if (S > 1) (void)hipMemsetAsync(dacq, 0, sizeof(double) * M, s);
    for (int sm = 0; sm + 1 < S; ++sm)
        hipLaunchKernelGGL(ei_accumulate_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dmu + pm * sm, dvar + pm * sm, M, M, par,
                           dcoef, dymax, dacq);
    hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, dmu + pm * (S - 1), dvar + pm * (S - 1), M, M,
                       par, dcoef, dymax, dacq, S > 1 ? 1 : 0, 1.0 / S, valid_mask ? dmask : nullptr, hres, 0ull);
    if (acq_out) (void)hipMemcpyAsync(acq_out, dacq, sizeof(double) * M, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
    if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
    if (max_out) *max_out = hres[0];
    return BOSS_OK;
}

static int device_index_of(const Multi& m, const Ctx* c) {
    for (int g = 0; g < m.G; ++g)
        if (m.ctx[g] == c) return g;
    return -1;
}

extern "C" int boss_multi_acq_ei_outputs(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                         const double* fit_coefs, const double* y_max, int has_best, double best,
                                         const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    if (P < 1 || S < 1 || M < 1 || !gps || !Xs || !fit_coefs) return fail(BOSS_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    int rc = multi_ready(1);
    if (rc) return rc;
    Multi& m = g_multi;
    const size_t PS = (size_t)P * S, pm = (size_t)P * M;
    std::vector<int> owner(PS);
    int d = 0;
    for (size_t i = 0; i < PS; ++i) {
        if (!gps[i]) return fail(BOSS_E_INVALID, "NULL posterior handle");
        NOT_FOR_KPROG(gps[i]);
        if (!gps[i]->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
        owner[i] = device_index_of(m, gps[i]->ctx);
        if (owner[i] < 0) return fail(BOSS_E_INVALID, "handle lives on a device boss_init did not open");
        d = gps[i]->d;
    }
    // every device: a zero-filled [S][2][P][M] block (mu rows then var rows of each sample); owners fill their rows
    const size_t count = 2 * pm * S;
    rc = on_devices(m.G, [&](int g) -> int {
        Ctx* c = m.ctx[g];
        HIPCHK(hipSetDevice(m.ctx[g]->device));
        int r = ws_reserve(m.red[g], sizeof(double) * (count + M));
        if (r) return r;
        double* buf = (double*)m.red[g].p;
        HIPCHK(hipMemsetAsync(buf, 0, sizeof(double) * count, c->stream));
        bool any = false;
        for (size_t i = 0; i < PS; ++i) any |= owner[i] == g;
        if (!any) return BOSS_OK;
        boss_cand_t* cd = nullptr;
        r = boss_cand_create(g, d, M, Xs, &cd);
        if (r) return r;
        {
            std::lock_guard<std::mutex> lkc(c->mtx);
            double* dmean = nullptr;
            std::vector<double> hrow(M);
            if (mean_Xs) {
                r = ws_reserve(c->pred, sizeof(double) * M);
                dmean = (double*)c->pred.p;
            }
            for (int sm = 0; sm < S && !r; ++sm)
                for (int p = 0; p < P && !r; ++p) {
                    if (owner[p + (size_t)P * sm] != g) continue;
                    if (mean_Xs) {
                        for (int j = 0; j < M; ++j) hrow[j] = mean_Xs[p + (size_t)P * (j + (size_t)M * sm)];
                        (void)hipMemcpyAsync(dmean, hrow.data(), sizeof(double) * M, hipMemcpyHostToDevice, c->stream);
                        (void)hipStreamSynchronize(c->stream);
                    }
                    double* mu = buf + 2 * pm * sm + (size_t)p * M;
                    r = predict_enqueue(gps[p + (size_t)P * sm], cd, dmean, mu, mu + pm);
                }
            (void)hipStreamSynchronize(c->stream);
        }
        std::string keep = g_last_error;
        boss_cand_free(cd);
        g_last_error = keep;
        return r;
    });
    if (rc) return rc;
    rc = multi_allreduce(m, count);                          // x + 0 + ... + 0 is exact: every device now holds every row
    if (rc) return rc;
    const int root = owner[0];
    HIPCHK(hipSetDevice(m.ctx[root]->device));
    Ctx* c = m.ctx[root];
    std::lock_guard<std::mutex> lkc(c->mtx);
    // [S][2][P][M]  ->  the epilogue wants mu[S][P][M] and var[S][P][M] with a common sample stride: pass per-sample pointers
    double* buf = (double*)m.red[root].p;
    double* dacq = buf + count;
    if (S == 1) {
        rc = moments_epilogue_dev(c, P, 1, M, buf, buf + pm, dacq, fit_coefs, y_max, has_best, best, valid_mask, acq_out, argmax_out, max_out);
    } else {
        // regroup on the device: mu rows of all samples first, then the var rows
        rc = ws_reserve(c->vscratch, sizeof(double) * count);
        if (rc) return rc;
        double* re = (double*)c->vscratch.p;
        for (int sm = 0; sm < S; ++sm) {
            (void)hipMemcpyAsync(re + pm * sm, buf + 2 * pm * sm, sizeof(double) * pm, hipMemcpyDeviceToDevice, c->stream);
            (void)hipMemcpyAsync(re + pm * S + pm * sm, buf + 2 * pm * sm + pm, sizeof(double) * pm, hipMemcpyDeviceToDevice, c->stream);
        }
        rc = moments_epilogue_dev(c, P, S, M, re, re + pm * S, dacq, fit_coefs, y_max, has_best, best, valid_mask, acq_out, argmax_out, max_out);
    }
    for (int g = 0; g < m.G; ++g) {                          // the other devices' share of the collective has drained too
        (void)hipSetDevice(m.ctx[g]->device);
        (void)hipStreamSynchronize(m.ctx[g]->stream);
    }
    return rc;
}

extern "C" int boss_multi_acq_ei_samples(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                                         const double* fit_coefs, const double* y_max, int has_best, double best,
                                         const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out) {
    if (P < 1 || S < 1 || M < 1 || !gps || !Xs || !fit_coefs) return fail(BOSS_E_INVALID, "bad arguments");
    std::lock_guard<std::mutex> lk(g_multi_mtx);
    int rc = multi_ready(1);
    if (rc) return rc;
    Multi& m = g_multi;
    std::vector<int> owner(S);
    int d = 0;
    for (int sm = 0; sm < S; ++sm)
        for (int p = 0; p < P; ++p) {
            const boss_gp* h = gps[p + (size_t)P * sm];
            if (!h) return fail(BOSS_E_INVALID, "NULL posterior handle");
            NOT_FOR_KPROG(h);
            if (!h->fitted) return fail(BOSS_E_NOT_FITTED, "handle has no valid factorisation");
            const int o = device_index_of(m, h->ctx);
            if (o < 0) return fail(BOSS_E_INVALID, "handle lives on a device boss_init did not open");
            if (p == 0) owner[sm] = o;
            else if (owner[sm] != o) return fail(BOSS_E_INVALID, "all outputs of one hyper-parameter sample must live on one device");
            d = h->d;
        }
    // every device: Σ over ITS samples of acq_s(x_j) into a zero-filled M-vector
    rc = on_devices(m.G, [&](int g) -> int {
        Ctx* c = m.ctx[g];
        HIPCHK(hipSetDevice(m.ctx[g]->device));
        int r = ws_reserve(m.red[g], sizeof(double) * M);
        if (r) return r;
        double* dsum = (double*)m.red[g].p;
        HIPCHK(hipMemsetAsync(dsum, 0, sizeof(double) * M, c->stream));
        bool any = false;
        for (int sm = 0; sm < S; ++sm) any |= owner[sm] == g;
        if (!any) return BOSS_OK;
        boss_cand_t* cd = nullptr;
        r = boss_cand_create(g, d, M, Xs, &cd);
        if (r) return r;
        {
            std::lock_guard<std::mutex> lkc(c->mtx);
            hipStream_t s = c->stream;
            const size_t pm = (size_t)P * M;
            r = ws_reserve(c->acq, sizeof(double) * (3 * pm + 2 * (size_t)P));
            double* dmu = (double*)c->acq.p;
            double* dvar = dmu + pm;
            double* dmean = dvar + pm;
            double* dcoef = dmean + pm;
            double* dymax = dcoef + P;
            EiPar par;
            if (!r) r = ei_params(c, s, P, fit_coefs, y_max, has_best, best, &par, dcoef, dymax);
            std::vector<double> hmean;
            for (int sm = 0; sm < S && !r; ++sm) {
                if (owner[sm] != g) continue;
                if (par.mode != 0) {
                    if (mean_Xs) {
                        hmean.resize(pm);
                        for (int j = 0; j < M; ++j)
                            for (int p = 0; p < P; ++p) hmean[(size_t)p * M + j] = mean_Xs[p + (size_t)P * (j + (size_t)M * sm)];
                        (void)hipMemcpyAsync(dmean, hmean.data(), sizeof(double) * pm, hipMemcpyHostToDevice, s);
                        (void)hipStreamSynchronize(s);
                    }
                    for (int p = 0; p < P && !r; ++p)
                        r = predict_enqueue(gps[p + (size_t)P * sm], cd, mean_Xs ? dmean + (size_t)p * M : nullptr, dmu + (size_t)p * M,
                                            dvar + (size_t)p * M);
                }
                if (!r)
                    hipLaunchKernelGGL(ei_accumulate_kernel, dim3((M + 255) / 256), dim3(256), 0, s, dmu, dvar, M, M, par, dcoef, dymax,
                                       dsum);
            }
            (void)hipStreamSynchronize(s);
        }
        std::string keep = g_last_error;
        boss_cand_free(cd);
        g_last_error = keep;
        return r;
    });
    if (rc) return rc;
    rc = multi_allreduce(m, (size_t)M);
    if (rc) return rc;
    // root: /S, mask, arg-max — the epilogue kernel with an empty "last sample" (mode 0 contributes exactly 0)
    const int root = owner[0];
    HIPCHK(hipSetDevice(m.ctx[root]->device));
    Ctx* c = m.ctx[root];
    {
        std::lock_guard<std::mutex> lkc(c->mtx);
        hipStream_t s = c->stream;
        rc = ws_reserve(c->acq, sizeof(double) * 4 + M + 64);
        if (rc) return rc;
        unsigned char* dmask = (unsigned char*)((double*)c->acq.p + 4);
        double* hres = (double*)c->pinned;
        double* dsum = (double*)m.red[root].p;
        EiPar par;
        par.P = 1;
        par.mode = 0;
        par.best = 0.0;
        if (valid_mask) (void)hipMemcpyAsync(dmask, valid_mask, M, hipMemcpyHostToDevice, s);
        const double* unused = (const double*)c->acq.p;      // mode 0 reads no moments
        hipLaunchKernelGGL(acq_epilogue_kernel, dim3(1), dim3(ACQ_EPI_THREADS), 0, s, unused, unused, M, M, par,
                           (const double*)nullptr, (const double*)nullptr, dsum, 1, 1.0 / S, valid_mask ? dmask : nullptr, hres, 0ull);
        if (acq_out) (void)hipMemcpyAsync(acq_out, dsum, sizeof(double) * M, hipMemcpyDeviceToHost, s);
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(BOSS_E_NO_DEVICE, hipGetErrorString(e));
        if (argmax_out) std::memcpy(argmax_out, &hres[1], sizeof(long));
        if (max_out) *max_out = hres[0];
    }
    for (int g = 0; g < m.G; ++g) {
        (void)hipSetDevice(m.ctx[g]->device);
        (void)hipStreamSynchronize(m.ctx[g]->stream);
    }
    return BOSS_OK;
}

extern "C" int boss_multi_loglike_batch(int G, int kernel, int d, int N, const double* X, const double* y, const double* mean_X,
                                        int mean_stride, const unsigned char* discrete, int S, const double* lengthscales,
                                        const double* amplitudes, const double* noise_stds, double* ll_out, int* status_out) {
    if (S < 0 || !ll_out) return fail(BOSS_E_INVALID, "bad arguments");
    {
        std::lock_guard<std::mutex> lk(g_multi_mtx);
        int rc = multi_ready(G);
        if (rc) return rc;
    }
    if (S == 0) return BOSS_OK;
    if (!lengthscales || !amplitudes || !noise_stds) return fail(BOSS_E_INVALID, "NULL hyper-parameter array");
    return on_devices(G, [&](int g) -> int {
        long lo, hi;
        shard_range(S, g, G, &lo, &hi);
        if (hi == lo) return BOSS_OK;
        const double* mx = mean_X ? (mean_stride ? mean_X + (size_t)mean_stride * lo : mean_X) : nullptr;
        return boss_gp_loglike_batch(g, kernel, d, N, X, y, mx, mean_stride, discrete, (int)(hi - lo), lengthscales + (size_t)d * lo,
                                     amplitudes + lo, noise_stds + lo, ll_out + lo, status_out ? status_out + lo : nullptr);
    });
}
