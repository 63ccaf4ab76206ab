"""The measurements behind the arg-max-only acquisition path's constants, as records (not thresholds).

  python tools/acq_prune_slack.py [--out profiles/acq_prune_slack.jsonl] [--slack 1.0]
  python tools/acq_prune_slack.py --sweep

Default: over the hyper-parameter grid of the regimes tests (tests/golden/make_regimes.py: 3 kernels × λ/√d ∈ {0.01, 0.1, 0.5, 3, 30} ×
α ∈ {0.05, 1.2, 30} × σ ∈ {1e-3, 0.05, 2}) at N = 1024, d = 3, M = 4131 (130 tiles: g.predict takes the fused kernel) and
s ∈ {1, 2}, one line per case: the path report of the pruned call, whether its arg-max equals the full call's,
rel_mu = max|μ_a − μ_fused| / (max|μ| + |best| + α), rel_var = max(σ²_fused − σ²_s) / α², min(ub − acq).  The slack constants in
csrc/host_prune.inc are 100 × the largest rel_mu / rel_var of such a run.  --slack scales them for the run (0: none; the run-time
mean check then fires wherever a finished mean differs from μ_a at all).

--sweep: at the benchmark's shape (N = 4096, d = 8, M = 8192) the acquisition call directly behind an update, median of 50, for
s ∈ {1, 2, 4} at K = 64 and K ∈ {32, 64, 128} at s = 2, beside the same factorisation again (a cached) and the full kernel.
The alternating runs of the two commits are plain `python bench.py --gpus 1 --steps 50 --warmup 5`, one line each."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def problem(N, d, M, seed=0):
    rng = np.random.default_rng(100 + seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = np.random.default_rng(200 + seed).uniform(0, 1, (d, M))
    return X, y, Xs


def grid(api, out, slack):
    N, d, M = 1024, 3, 4131
    X, y, Xs = problem(N, d, M)
    cand = api.Candidates(Xs)
    best = float(y.max())
    worst_mu, worst_var = (-1.0, None), (-np.inf, None)
    with open(out, "w") as f:
        for kernel in ("matern32", "matern52", "sqexp"):
            g = api.GP(X, y, kernel)
            for lr in (0.01, 0.1, 0.5, 3.0, 30.0):
                for amp in (0.05, 1.2, 30.0):
                    for sig in (1e-3, 0.05, 2.0):
                        g.update(np.full(d, lr * np.sqrt(d)), amp, sig)
                        mu, var = g.predict(Xs)
                        acq, am_f, _ = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=True)
                        for s in (1, 2):
                            # (cap >= M − K: where EI underflows, T = 0 and everything survives; only the mean check falls back)
                            api._acq_prune_set(0, min_tiles=0, K=64, s=s, cap=4096, slack=slack)
                            for _ in range(66):            # (past whatever pause an earlier fallback left on the handle)
                                _, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
                                rep = api._acq_path(0)
                                if rep[0] != 3:
                                    break
                            assert rep[0] in (1, 2), rep
                            mua, vs, ub = api._acq_prune_bounds(M)
                            rel_mu = float(np.max(np.abs(mua - mu)) / (np.max(np.abs(mu)) + abs(best) + amp))
                            rel_var = float(np.max(var - vs) / amp ** 2)
                            line = {"kernel": kernel, "lam_rel": lr, "amp": amp, "sig": sig, "s": s, "path": list(rep), "same": bool(am == am_f),
                                    "rel_mu": rel_mu, "rel_var": rel_var, "min_ub_minus_acq": float(np.nanmin(ub - acq))}
                            f.write(json.dumps(line) + "\n")
                            f.flush()
                            name = f"{kernel} lam_rel {lr} amp {amp} sig {sig} s {s}"
                            if rel_mu > worst_mu[0]:
                                worst_mu = (rel_mu, name)
                            if rel_var > worst_var[0]:
                                worst_var = (rel_var, name)
    api._acq_prune_set(0, min_tiles=-2, K=-2, s=-2, cap=-2, slack=1.0)
    print(f"largest rel_mu {worst_mu[0]:.3e} ({worst_mu[1]}); largest rel_var {worst_var[0]:.3e} ({worst_var[1]}); rows in {out}")


def sweep(api):
    d, N, M = 8, 4096, 8192
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = rng.uniform(0, 1, (d, M))
    g = api.GP(X, y, "matern52")
    cand = api.Candidates(Xs)
    best = float(y.max())

    def timed(update_first, want_acq=False, n=50):
        ts = []
        for i in range(n + 3):
            if update_first:
                g.update(np.full(d, 0.5), 1.0, 0.05 + 1e-6 * (i % 2))
            t = time.perf_counter()
            api.acq_ei([[g]], cand, [1.0], None, best, want_acq=want_acq)
            ts.append(time.perf_counter() - t)
        return float(np.median(ts[3:]) * 1e3)

    g.update(np.full(d, 0.5), 1.0, 0.05)
    for s, K in ((1, 64), (2, 64), (4, 64), (2, 32), (2, 128)):
        api._acq_prune_set(0, K=K, s=s)
        print(json.dumps({"s": s, "K": K, "ms_acq_behind_update": timed(True), "path": list(api._acq_path(0))}), flush=True)
    api._acq_prune_set(0, K=-2, s=-2)
    print(json.dumps({"a_cached_ms": timed(False), "full_kernel_ms": timed(False, want_acq=True)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "acq_prune_slack.jsonl"))
    ap.add_argument("--slack", type=float, default=1.0)
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api
    api.load_library()
    if args.sweep:
        sweep(api)
    else:
        grid(api, args.out, args.slack)


if __name__ == "__main__":
    main()
