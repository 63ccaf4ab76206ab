"""What the gradient through the prior mean costs: boss_gp_loglike_grad_batch_mean (per-set Jacobians, dtheta only) beside
boss_gp_loglike_grad_batch at the same arguments, and the host-to-device copy of the Jacobians on its own; ms per call.

  python tools/semipar_llgrad_times.py --label run1 --out profiles/semipar_llgrad.jsonl

The driver starts ONE process per shape (--only N:S is that process), each under a time limit, and stops at the first that fails.
In that process the three measurements alternate call by call (old, new, copy, old, new, copy, …) after two warm-up rounds, 20
rounds, each with a host clock around work that ends in a synchronisation; a line carries p50 / min / max of each and the source
hash of the library.  Both entry points are called at the C ABI with arrays laid out beforehand, so neither pays for a conversion.
Shapes: (N, S) = (20, 20), (1024, 8), (1024, 64), (2048, 8), (2048, 64), d = 4, T = 8.  `--only fitter` times one round of
HipGradientMAP's objective (20 trial points, P = 2, N = 100, d = 2, T = 3) over a Semiparametric model beside the same round
with the mean held fixed at one θ.  Three runs (labels run1..run3) give the spread: max − min of the old call's three p50s."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(20, 20), (1024, 8), (1024, 64), (2048, 8), (2048, 64)]
D, T = 4, 8


def stats(ts):
    return dict(p50_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))


def ms(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def one_shape(a, api, stamp):
    N, S = (int(v) for v in a.only.split(":"))
    rng = np.random.default_rng(N * 1000 + S)
    X = np.asfortranarray(rng.uniform(0, 1, (D, N)))
    y = np.sin(3 * X).sum(0) / np.sqrt(D) + 0.1 * rng.standard_normal(N)
    lam = np.asfortranarray(rng.uniform(0.3, 0.9, (D, S)) * np.sqrt(D))
    amp, sig = rng.uniform(0.7, 1.4, S), rng.uniform(0.05, 0.15, S)
    means = np.ascontiguousarray(0.1 * X[0][None, :] + 0.01 * np.arange(S)[:, None])
    J = rng.standard_normal((S, T, N))                          # set after set, each N×T column-major
    ll, gr, dth, st = np.zeros(S), np.zeros((D + 2, S), order="F"), np.zeros((T, S), order="F"), np.zeros(S, dtype=np.int32)
    lib = api.load_library()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    stp = st.ctypes.data_as(C.POINTER(C.c_int))
    k = api.KERNELS["matern52"]

    def checked(rc):
        if rc != 0:
            raise RuntimeError(f"status {rc}: {lib.boss_last_error().decode()}")

    def old():
        checked(lib.boss_gp_loglike_grad_batch(0, k, D, N, dp(X), dp(y), dp(means), N, None, S, dp(lam), dp(amp), dp(sig), dp(ll), dp(gr), stp))

    def new():
        checked(lib.boss_gp_loglike_grad_batch_mean(0, k, D, N, dp(X), dp(y), dp(means), N, None, S, dp(lam), dp(amp), dp(sig), T, dp(J), N * T,
                                                    dp(ll), dp(gr), None, dp(dth), stp))
    old()                                                       # (the library sets the device up before anything else touches it)
    # the copy on its own: pageable host memory to the device through the HIP runtime the library runs on, blocking
    hip, Jdev = None, C.c_void_p()
    try:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if hip.hipMalloc(C.byref(Jdev), J.nbytes) != 0:
            hip = None
    except OSError:
        hip = None                                              # (the copy is then reported as not measured)

    def copy():
        if hip is not None and (hip.hipMemcpy(Jdev, J.ctypes.data_as(C.c_void_p), J.nbytes, 1) != 0 or hip.hipDeviceSynchronize() != 0):
            raise RuntimeError("hipMemcpy failed")
    for _ in range(2):
        old(), new(), copy()
    ok = bool((st == 0).all())
    to, tn, tc = [], [], []
    for _ in range(a.reps):
        to.append(ms(old))
        tn.append(ms(new))
        tc.append(ms(copy))
    return dict(N=N, S=S, d=D, T=T, calls=a.reps, all_pd=ok, jac_mib=J.nbytes / 2 ** 20, old=stats(to), new=stats(tn),
                jac_copy=stats(tc) if hip is not None else "not measured", label=a.label, source_hash=stamp)


def fitter_round(a, api, stamp):
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    rng = np.random.default_rng(11)
    d, N, P, S = 2, 100, 2, 20
    par = lambda x, th: np.array([th[0] + th[1] * x[0] + np.cos(th[2] * x[1]), 0.5 * th[0] - th[1] * x[1] + np.cos(th[2] * x[0])])   # noqa: E731
    jac = lambda x, th: np.array([[1.0, x[0], -x[1] * np.sin(th[2] * x[1])], [0.5, -x[1], -x[0] * np.sin(th[2] * x[0])]])           # noqa: E731
    th0 = np.array([0.8, -0.6, 1.3])
    X = rng.uniform(0, 2, (d, N))
    Y = np.stack([[par(X[:, j], th0)[i] for j in range(N)] for i in range(P)]) + 0.05 * rng.standard_normal((P, N))
    pri = dict(lengthscale_priors=[B.MvLogNormal([-0.5, -0.5], [0.3, 0.3])] * P, amplitude_priors=[B.LogNormal(-1.0, 0.3)] * P,
               noise_std_priors=[B.LogNormal(-3.0, 0.3)] * P)
    semi = B.HipGaussianProcess(parametric=par, parametric_jac=jac, theta_priors=[B.Normal(0.0, 2.0)] * 3, **pri)
    numeric = B.HipGaussianProcess(parametric=par, theta_priors=[B.Normal(0.0, 2.0)] * 3, **pri)
    fixed = B.HipGaussianProcess(mean=lambda x: par(x, th0), **pri)
    data = B.ExperimentData(X, Y)
    plist = [semi.params_sampler()(rng) for _ in range(S)]
    flist = [B.HipGPParams(p.lengthscales, p.amplitudes, p.noise_std) for p in plist]
    fit = B.HipGradientMAP()
    rounds = {"semiparametric": lambda: fit._objective_semiparametric(semi, semi.params_loglike(), data, plist),
              "semiparametric_numeric_jac": lambda: fit._objective_semiparametric(numeric, numeric.params_loglike(), data, plist),
              "fixed_mean": lambda: fit._objective_batch(fixed, fixed.params_loglike(), data, flist)}
    for _ in range(2):
        for r in rounds.values():
            r()
    ts = {name: [] for name in rounds}
    for _ in range(a.reps):
        for name, r in rounds.items():
            ts[name].append(ms(r))
    return dict(fitter_round=True, N=N, S=S, d=d, P=P, T=3, calls=a.reps, label=a.label, source_hash=stamp,
                **{name: stats(v) for name, v in ts.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="N:S or `fitter` — time this in this process")
    ap.add_argument("--step-timeout", type=float, default=150.0)
    a = ap.parse_args()
    if a.only:
        sys.path.insert(0, ROOT)
        from boss_jl_amd import api
        api.load_library()
        side = api.LIB_PATH + ".srchash"
        stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
        rec = fitter_round(a, api, stamp) if a.only == "fitter" else one_shape(a, api, stamp)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        return
    for only in [f"{N}:{S}" for N, S in SHAPES] + ["fitter"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--label", a.label, "--reps", str(a.reps), "--only", only]
        if a.out:
            cmd += ["--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                                              # a failed or hung shape ends the run: nothing more is started
            print(f"[semipar-llgrad-times] {only} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
