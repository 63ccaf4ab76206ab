"""What a device warp costs and what it saves: the one-call warped acquisition beside the plain calls on already-warped candidates
and beside the plain-closure HipTransformedModel.

  python tools/warp_times.py --label run1 --out profiles/warp.jsonl

One process, every figure p50 / min / max of --reps calls (20) after two warm-up calls, a host clock around the WHOLE Python call (it
ends synchronised); the variants of one measurement alternate call by call.  BASELINE config 4's shape: N = 2048, d = 6, P = 2, a log
input warp on every coordinate and a sliced affine output transform.
(a) 8192 candidates, values:     boss_acq_ei_warp on user-space candidates | boss_acq_ei on a resident candidate set of the already
    warped X_ (the difference is what the warp costs) | the plain-closure model's host path (what it saves).
(b) 224 ascent starts, gradient: boss_acq_ei_grad_warp | boss_acq_ei_grad on the already warped X_ (no Jacobian is applied there: a
    lower bound of the work, not the same result)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    return dict(p50_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), calls=len(ts))


def alternate(calls, reps):
    for _ in range(2):
        for c in calls.values():
            c()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, c in calls.items():
            t = time.perf_counter()
            c()
            ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: stats(v) for k, v in ts.items()}


AFFINE = ((2.0, 1.0), (0.5, -0.3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    from boss_jl_amd.transformed import warped_acquisition_values
    api.load_library()
    if api.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    rng = np.random.default_rng(0)
    d, N, P = 6, (128 if a.small else 2048), 2
    M, starts = (256 if a.small else 8192), (32 if a.small else 224)
    win = lambda x: np.log(x + 0.1)                                                      # noqa: E731
    fw = [(lambda y, s, a_=a_, b_=b_: (a_ * y + b_, a_ * s)) for a_, b_ in AFFINE]
    bw = [(lambda y, a_=a_, b_=b_: (y - b_) / a_) for a_, b_ in AFFINE]
    X = rng.uniform(0, 1, (d, N))
    X_ = np.log(X + 0.1)
    Y_ = np.stack([np.sin(3 * X_).sum(0) / np.sqrt(d), X_[0] - X_[1] + 0.2 * np.cos(4 * X_[2])]) + 0.05 * rng.standard_normal((P, N))
    Y = np.stack([a_ * Y_[i] + b_ for i, (a_, b_) in enumerate(AFFINE)])
    params = B.HipGPParams(np.full((d, P), 0.9), [1.0, 1.0], [0.05, 0.05])
    base = lambda: B.HipGaussianProcess([None] * P, [None] * P, [None] * P)             # noqa: E731
    mk = lambda m: B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([0.7, -0.2])), m,      # noqa: E731
                                 B.ExperimentData(X, Y), y_max=[np.inf, 2.0], params=params)
    p_dev = mk(B.HipTransformedModel(base(), B.DeviceInputTransform(win, d, d), B.DeviceSlicedOutputTransform(fw, bw)))
    p_host = mk(B.HipTransformedModel(base(), B.InputTransform(win), B.SlicedOutputTransform(fw, bw)))
    post_d = p_dev.model.model_posterior(params, p_dev.data)
    post_h = p_host.model.model_posterior(params, p_host.data)
    gps = [[s.gp for s in post_d.base.slices]]
    w = p_dev.model.warp
    rec = dict(label=a.label, source_hash=stamp, reps=a.reps, small=a.small, N=N, d=d, P=P)

    Xs = np.asfortranarray(rng.uniform(0, 1, (d, M)))
    cand = api.Candidates(np.asfortranarray(np.log(Xs + 0.1)))
    coefs, ymax, best = [0.7, -0.2], [np.inf, 2.0], float(Y[0].max())
    rec["values"] = dict(candidates=M, **alternate({
        "acq_ei_warp": lambda: w.acq_ei(gps, Xs, coefs, ymax, best, None, None, want_acq=False),
        "acq_ei_on_warped": lambda: api.acq_ei(gps, cand, coefs, ymax, best, None, None, want_acq=False),
        "plain_closure_model": lambda: warped_acquisition_values(p_host, [post_h], Xs)}, a.reps))
    X0 = np.asfortranarray(rng.uniform(0, 1, (d, starts)))
    X0_ = np.asfortranarray(np.log(X0 + 0.1))
    rec["gradients"] = dict(starts=starts, **alternate({
        "acq_ei_grad_warp": lambda: w.acq_ei_grad(gps, X0, coefs, ymax, best),
        "acq_ei_grad_on_warped": lambda: api.acq_ei_grad(gps[0], X0_, coefs, ymax, best)}, a.reps))
    cand.close()
    post_d.close()
    post_h.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
