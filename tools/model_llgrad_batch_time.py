"""Batched likelihood GRADIENTS of the gradient-observation and the nonstationary model against the loop they replace: ms per call.

  python tools/model_llgrad_batch_time.py --mode batched            one boss_ggp_loglike_grad_batch / boss_ngp_loglike_grad_batch call
  python tools/model_llgrad_batch_time.py --mode loop [--lib PATH]  S × (update + loglike_grad) on ONE resident handle — what
                                                                    HipGradientMAP._objective_gradient_model ran before the batched
                                                                    call; --lib times another build of the library (the parent
                                                                    commit's) with this script

The driver starts ONE process per shape (--only model:rows:S is that process), each under a time limit, and stops at the first
that fails.  A shape is warmed up (2 calls), then timed for 20 calls (fewer, at least 5, once it has used --budget seconds) with a
host clock around work that ends in a synchronisation; its line carries p50 / min / max and the source hash of the library it
timed.  Gradient model: n(1+d) = 60, 240, 1017, 2043, 4095 rows (GRAD_SHAPES); nonstationary: N = 256, 1024, 2048 at d = 4;
S = 8 and 64.  Three runs of each mode (labels this-runK / parent-runK) give the ranges of DESIGN.md §4.2."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_SHAPES = [(20, 2), (48, 4), (113, 8), (227, 8), (455, 8)]     # (n, d): 60, 240, 1017, 2043, 4095 rows
NS_SHAPES = [(4, 256), (4, 1024), (4, 2048)]                       # (d, N)
SETS = (8, 64)


def timed(call, reps, budget):
    for _ in range(2):
        call()
    ts, t0 = [], time.perf_counter()
    while len(ts) < reps and (len(ts) < 5 or time.perf_counter() - t0 < budget):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def one_shape(a):
    model, rows, S = a.only.split(":")
    rows, S = int(rows), int(S)
    if a.lib:
        os.environ["BOSS_LIB_PATH"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    from boss_jl_amd import api
    api.load_library()
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    rng = np.random.default_rng(rows * 1000 + S)
    if model == "gradient":
        n, d = next((n, d) for n, d in GRAD_SHAPES if n * (1 + d) == rows)
        X = rng.uniform(0, 1, (d, n))
        w = rng.uniform(0.5, 2.0, d)
        y, dY = np.sin(X.T @ w), w[:, None] * np.cos(X.T @ w)[None, :]
        lam = rng.uniform(0.3, 1.5, (d, S))
        amp, sig, sgd = rng.uniform(0.5, 2, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
        if a.mode == "batched":
            call = lambda: api.ggp_loglike_grad_batch(X, y, dY, "matern52", lam, amp, sig, sgd)            # noqa: E731
            ok = bool((call()[1] == 0).all())
        else:
            g = api.GradGP(X, y, dY, "matern52")

            def call():
                out = []
                for s in range(S):
                    g.update(lam[:, s], amp[s], sig[s], sgd[s])
                    out.append(g.loglike_grad())
                return out
            ok = bool(np.isfinite([r[0] for r in call()]).all())
        shape = dict(model=model, rows=rows, n=n, d=d, S=S)
    else:
        d, N = next((d, N) for d, N in NS_SHAPES if N == rows)
        X = rng.uniform(0, 1, (d, N))
        y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
        lam0 = 0.25 + 0.5 * X ** 2 + 0.1 * np.arange(1, d + 1)[:, None]
        amp0, noi0 = 1.0 + 0.4 * np.sin(3 * X[0]), 0.03 + 0.05 * X[-1] ** 2
        c, am, nz = rng.uniform(0.7, 1.6, S), rng.uniform(0.6, 1.8, S), rng.uniform(1, 3, S)
        lam = np.asfortranarray(lam0[:, :, None] * c)
        amp, noi = np.asfortranarray(amp0[:, None] * am), np.asfortranarray(noi0[:, None] * nz)
        if a.mode == "batched":
            call = lambda: api.ngp_loglike_grad_batch(X, y, lam, amp, noi)                                 # noqa: E731
            ok = bool((call()[1] == 0).all())
        else:
            g = api.GibbsGP(X, y)
            per_set = [(np.asfortranarray(lam[:, :, s]), np.ascontiguousarray(amp[:, s]), np.ascontiguousarray(noi[:, s])) for s in range(S)]

            def call():
                out = []
                for p in per_set:
                    g.update(*p)
                    out.append(g.loglike_grad())
                return out
            ok = bool(np.isfinite([r[0] for r in call()]).all())
        shape = dict(model=model, rows=rows, d=d, S=S)
    ts = timed(call, a.reps, a.budget)
    rec = dict(shape, calls=len(ts), p50_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts), all_pd=ok, mode=a.mode, label=a.label,
               source_hash=stamp)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batched", "loop"), required=True)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="model:rows:S — time this shape in this process")
    ap.add_argument("--step-timeout", type=float, default=120.0)
    a = ap.parse_args()
    if a.only:
        return one_shape(a)
    shapes = [("gradient", n * (1 + d), S) for n, d in GRAD_SHAPES for S in SETS] + [("nonstationary", N, S) for _, N in NS_SHAPES for S in SETS]
    for model, rows, S in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", a.mode, "--label", a.label, "--reps", str(a.reps), "--budget",
               str(a.budget), "--only", f"{model}:{rows}:{S}"]
        if a.lib:
            cmd += ["--lib", a.lib]
        if a.out:
            cmd += ["--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                                              # a failed or hung shape ends the run: nothing more is started
            print(f"[model-llgrad-batch-time] {model}:{rows}:{S} ended with status {rc}; stopping", file=sys.stderr, flush=True)
            sys.exit(rc if rc > 0 else 1)


if __name__ == "__main__":
    main()
