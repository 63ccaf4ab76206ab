"""cov_probe.py — times the posterior covariance of the gradient-observation and nonstationary models on one MI355X
(boss_ggp_predict_cov / boss_ngp_predict_cov: cov_syrk_partial_kernel + cov_finish_kernel) next to the plain model's
boss_gp_predict_cov (VALU predict_cov_kernel) at the same padded system size Np and candidate count M.

  python tools/cov_probe.py [--case NAME] [--calls K]          whole-call times (median of K after one warm-up call), the
                                                               device-to-host copy of the M×M result; one JSON line per case
  rocprofv3 --kernel-trace --stats -d DIR -o s -- python tools/cov_probe.py --case NAME --calls 3
                                                               kernel times, in a separate run (the trace slows the calls)
  python tools/cov_probe.py --summarize TIMES.jsonl STATSROOT  joins both: per case the kernel times of cov_syrk_partial_kernel,
                                                               cov_finish_kernel and predict_cov_kernel (STATSROOT/<case>/**/
                                                               *kernel_stats.csv) and the product step's TFLOP/s at
                                                               Np·M·(M+64) FLOP (64×64 lower-triangle blocks)
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (model, training points (n for gradient observations), x_dim, M)
CASES = {
    "ngp_N4096_M256": ("ngp", 4096, 8, 256),
    "ngp_N4096_M1024": ("ngp", 4096, 8, 1024),
    "ngp_N4096_M4096": ("ngp", 4096, 8, 4096),
    "ggp_n1024_M256": ("ggp", 1024, 8, 256),
    "ggp_n1024_M1024": ("ggp", 1024, 8, 1024),
    "ggp_n1024_M4096": ("ggp", 1024, 8, 4096),
    "ggp_n4096_M1024": ("ggp", 4096, 8, 1024),
}
PEAK_F64_MFMA_TF = 78.6


def _median_time(fn, calls):
    fn()                                                     # warm-up: workspaces, first-call paths
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _d2h_time(M, calls):
    """hipMemcpy of an M×M double matrix from the device into pageable host memory (what the entry points do last)."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    nbytes = 8 * M * M
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes)) == 0
    assert hip.hipMemset(dev, 0, C.c_size_t(nbytes)) == 0
    host = np.empty((M, M))

    def copy():
        assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, C.c_size_t(nbytes), 2) == 0   # hipMemcpyDeviceToHost
    try:
        return _median_time(copy, calls)
    finally:
        hip.hipFree(dev)


def run_case(name, calls):
    from boss_jl_amd import api
    model, n, d, M = CASES[name]
    rng = np.random.default_rng(7)
    Xs = np.asfortranarray(rng.uniform(0, 1, (d, M)))
    if model == "ggp":
        X = rng.uniform(0, 1, (d, n))
        w = np.linspace(1.0, 2.0, d)[:, None]
        y = np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(d)
        dY = 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(d)
        g = api.GradGP(X, y, dY, "matern52")
        g.update(np.full(d, 0.6), 1.0, 0.05, 0.1)
        call = lambda: g.predict_value_cov(Xs)               # noqa: E731
        Np = g.N
    else:
        X = rng.uniform(0, 1, (d, n))
        y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d)
        g = api.GibbsGP(X, y)
        g.update(0.4 + 0.3 * X, 1.0 + 0.2 * X[0], np.full(n, 0.05))
        lamS, ampS = 0.4 + 0.3 * Xs, 1.0 + 0.2 * Xs[0]
        call = lambda: g.predict_cov(Xs, lamS, ampS)         # noqa: E731
        Np = n
    Np = (Np + 255) // 256 * 256
    t_call = _median_time(call, calls)
    g.close()
    # the plain model at the same Np and M: the VALU covariance kernel
    Xp = rng.uniform(0, 1, (d, Np))
    gp = api.fit(Xp, np.sin(2 * np.pi * Xp).sum(0) / np.sqrt(d), "matern52", np.full(d, 0.6), 1.0, 0.05)
    t_plain = _median_time(lambda: gp.predict_cov(Xs), calls)
    gp.close()
    t_d2h = _d2h_time(M, calls)
    return {"case": name, "model": model, "d": d, "Np": Np, "M": M, "call_s": t_call, "plain_call_s": t_plain, "d2h_MxM_s": t_d2h}


def _stats(root):
    out = {}
    for f in glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            for k in ("cov_syrk_partial_kernel", "cov_finish_kernel", "predict_cov_kernel"):
                if k in row["Name"]:
                    c, tot = out.get(k, (0, 0.0))
                    out[k] = (c + int(row["Calls"]), tot + float(row["TotalDurationNs"]))
    return {k: tot / c * 1e-9 for k, (c, tot) in out.items() if c}


def summarize(times_path, stats_root):
    rows = []
    for line in open(times_path):
        line = line.strip()
        if not line.startswith("{"):
            continue
        r = json.loads(line)
        k = _stats(os.path.join(stats_root, r["case"]))
        r["syrk_kernel_s"] = k.get("cov_syrk_partial_kernel")
        r["finish_kernel_s"] = k.get("cov_finish_kernel")
        r["plain_predict_cov_kernel_s"] = k.get("predict_cov_kernel")
        flop = float(r["Np"]) * r["M"] * (r["M"] + 64)
        if r["syrk_kernel_s"]:
            r["syrk_TFLOPs"] = flop / r["syrk_kernel_s"] * 1e-12
            r["syrk_fraction_of_peak"] = r["syrk_TFLOPs"] / PEAK_F64_MFMA_TF
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all"] + list(CASES))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--summarize", nargs=2, metavar=("TIMES_JSONL", "STATS_ROOT"))
    a = ap.parse_args()
    if a.summarize:
        import __graft_entry__ as entry
        print(json.dumps({"source_hash": entry.source_hash()}))
        for r in summarize(*a.summarize):
            print(json.dumps(r))
        return
    from boss_jl_amd import api
    api.load_library()
    for name in (CASES if a.case == "all" else [a.case]):
        print(json.dumps(run_case(name, a.calls)), flush=True)


if __name__ == "__main__":
    main()
