"""Batched likelihoods of the gradient-observation and the nonstationary model against the loops they replace: ms per call.

  python tools/model_batch_time.py --mode batched            one boss_ggp_loglike_batch / boss_ngp_loglike_batch call for S sets
  python tools/model_batch_time.py --mode loop [--lib PATH]  S updates on ONE resident handle (boss_ggp_update / boss_ngp_update) —
                                                             what data_loglike_batch ran before the batched calls; --lib times
                                                             another build of the library (e.g. the parent commit's) with this script

One process per build and mode; every shape is warmed up (2 calls), then timed for 20 calls (fewer, at least 5, once a shape has
used --budget seconds) around work that ends in a synchronisation; the line carries p50 / min / max and the library's source hash.
Gradient model: n(1+d) = 60, 240, 1017, 2043, 4095 rows; nonstationary model: N = 256, 1024, 2048; S = 8, 64, 512 (S = 512 is
skipped where the loop alone would take minutes: from 2043 rows on).  --extra adds what the switch-over in
HipGradientGaussianProcess.data_loglike_batch needs beyond that: S = 2 at every size and an 8190-row gradient system.
--only model:rows:S runs one shape (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_SHAPES = [(20, 2), (48, 4), (113, 8), (227, 8), (455, 8)]     # (n, d): 60, 240, 1017, 2043, 4095 rows
NS_SHAPES = [(4, 256), (4, 1024), (4, 2048)]                       # (d, N)
SETS = (8, 64, 512)


def timed(call, reps, budget):
    for _ in range(2):
        call()
    ts, t0 = [], time.perf_counter()
    while len(ts) < reps and (len(ts) < 5 or time.perf_counter() - t0 < budget):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def update_or_inf(api, g, *p):
    try:
        return g.update(*p)
    except api.PosDefException:
        return -np.inf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("batched", "loop"), required=True)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-rows", type=int, default=1 << 30)
    ap.add_argument("--extra", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    grad_shapes = GRAD_SHAPES + ([(910, 8)] if a.extra else [])     # 8190 rows
    sets = ((2,) if a.extra else ()) + SETS
    only = None if a.only is None else (a.only.split(":")[0], int(a.only.split(":")[1]), int(a.only.split(":")[2]))

    def skip(model, rows, S):
        return (S == 512 and rows > 1100) or (only is not None and only != (model, rows, S))
    if a.lib:
        os.environ["BOSS_LIB_PATH"] = os.path.abspath(a.lib)
    sys.path.insert(0, ROOT)
    from boss_jl_amd import api
    api.load_library()
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        rec.update(mode=a.mode, label=a.label, source_hash=stamp)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rng = np.random.default_rng(0)
    for n, d in grad_shapes:
        rows = n * (1 + d)
        if rows > a.max_rows or (only is not None and only[:2] != ("gradient", rows)):
            continue
        X = rng.uniform(0, 1, (d, n))
        w = rng.uniform(0.5, 2.0, d)
        y, dY = np.sin(X.T @ w), w[:, None] * np.cos(X.T @ w)[None, :]
        g = api.GradGP(X, y, dY, "matern52") if a.mode == "loop" else None
        for S in sets:
            if skip("gradient", rows, S):
                continue
            lam = rng.uniform(0.3, 1.5, (d, S))
            amp, sig, sgd = rng.uniform(0.5, 2, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
            if a.mode == "batched":
                call = lambda: api.ggp_loglike_batch(X, y, dY, "matern52", lam, amp, sig, sgd)            # noqa: E731
                ll, st = call()
                ok = bool((st == 0).all())
            else:
                call = lambda: [update_or_inf(api, g, lam[:, s], amp[s], sig[s], sgd[s]) for s in range(S)]            # noqa: E731
                ok = bool(np.isfinite(call()).all())
            ts = timed(call, a.reps, a.budget)
            emit(dict(model="gradient", rows=rows, n=n, d=d, S=S, calls=len(ts), p50_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts),
                      all_pd=ok))
        if g is not None:
            g.close()
    for d, N in NS_SHAPES:
        if N > a.max_rows or (only is not None and only[:2] != ("nonstationary", N)):
            continue
        X = rng.uniform(0, 1, (d, N))
        y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
        lam0 = 0.25 + 0.5 * X ** 2 + 0.1 * np.arange(1, d + 1)[:, None]
        amp0, noi0 = 1.0 + 0.4 * np.sin(3 * X[0]), 0.03 + 0.05 * X[-1] ** 2
        g = api.GibbsGP(X, y) if a.mode == "loop" else None
        for S in sets:
            if skip("nonstationary", N, S):
                continue
            c, am, nz = rng.uniform(0.7, 1.6, S), rng.uniform(0.6, 1.8, S), rng.uniform(1, 3, S)
            lam = np.asfortranarray(lam0[:, :, None] * c)
            amp, noi = np.asfortranarray(amp0[:, None] * am), np.asfortranarray(noi0[:, None] * nz)
            if a.mode == "batched":
                call = lambda: api.ngp_loglike_batch(X, y, lam, amp, noi)                                 # noqa: E731
                ll, st = call()
                ok = bool((st == 0).all())
            else:
                per_set = [(np.asfortranarray(lam[:, :, s]), np.ascontiguousarray(amp[:, s]), np.ascontiguousarray(noi[:, s])) for s in range(S)]
                call = lambda: [update_or_inf(api, g, *p) for p in per_set]                                               # noqa: E731
                ok = bool(np.isfinite(call()).all())
            ts = timed(call, a.reps, a.budget)
            emit(dict(model="nonstationary", rows=N, d=d, S=S, calls=len(ts), p50_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts),
                      all_pd=ok))
        if g is not None:
            g.close()


if __name__ == "__main__":
    main()
