"""What an acquisition program costs on the device, beside the built-in EI it can spell and the host path a custom acquisition took.

  python tools/acq_prog_times.py --label run1 --out profiles/acq_prog.jsonl

Setup: N = 2048 observations, d = 6, P = 2 outputs, one posterior sample; 8192 candidates for values, 224 for gradients.  The
program is EI × feasibility spelled branch-free over q = [best, y_max_1, y_max_2] (muf and vf as sequential sums, z = (muf − best) /
sqrt(vf), (diff·Φ(z) + sf·φ(z)) · Π Φ((y_max_p − μ_p)/sqrt(σ²_p))), so the same handles answer the same question three ways.
Measured, each with a host clock around the WHOLE Python call (it ends synchronised), after two warm-up calls, p50 / min / max of
--reps calls (20); the three value calls alternate call by call, as do the two gradient calls:
  values      boss_acq_prog | boss_acq_ei | mean_and_var to the host + the numpy closure (what a custom acquisition did before)
  gradients   boss_acq_prog_grad | boss_acq_ei_grad
These are records, not pass marks."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, P, M_ACQ, M_GRAD = 2048, 6, 2, 8192, 224
COEFS, Y_MAX = [1.0, -0.5], [np.inf, 0.8]


def stats(ts):
    return dict(p50_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), calls=len(ts))


def ms(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    api.load_library()
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (D, N))
    Y = np.stack([np.sin(3 * X).sum(0) / np.sqrt(D), X[0] - X[1] + 0.2 * np.cos(4 * X[2])]) + 0.05 * rng.standard_normal((P, N))
    gps = []
    for p in range(P):
        g = api.GP(X, Y[p], "matern52")
        g.update(np.full(D, 0.5 + 0.1 * p), 1.0, 0.05)
        gps.append(g)
    c = np.asarray(COEFS)
    best = float(np.max(c @ Y[:, Y[1] <= Y_MAX[1]]))
    q = np.array([best] + Y_MAX)

    def ei_fp(mu, var, q):
        muf, vf = c[0] * mu[0], (c[0] * c[0]) * var[0]
        for p in range(1, P):
            muf, vf = muf + c[p] * mu[p], vf + (c[p] * c[p]) * var[p]
        sf, diff = np.sqrt(vf), muf - q[0]
        z = diff / sf
        acq = diff * B.normcdf(z) + sf * B.normpdf(z)
        for p in range(P):
            acq = acq * B.normcdf((q[1 + p] - mu[p]) / np.sqrt(var[p]))
        return acq
    prog = B.trace_acquisition(ei_fp, P, 1 + P)
    Xs = np.asfortranarray(rng.uniform(0, 1, (D, M_ACQ)))
    Xg = np.asfortranarray(rng.uniform(0, 1, (D, M_GRAD)))
    cand = api.Candidates(Xs)

    def host_path():
        mv = [g.predict(Xs) for g in gps]
        acq = ei_fp(np.stack([m for m, _ in mv]), np.stack([v for _, v in mv]), q)
        return acq, int(np.argmax(acq))
    values = {"acq_prog": lambda: api.acq_prog([gps], cand, prog, q, None, 0.0),
              "acq_ei": lambda: api.acq_ei([gps], cand, COEFS, Y_MAX, best),
              "host_numpy": host_path}
    grads = {"acq_prog_grad": lambda: api.acq_prog_grad([gps], Xg, prog, q, None, 0.0),
             "acq_ei_grad": lambda: api.acq_ei_grad(gps, Xg, COEFS, Y_MAX, best)}
    rec = {"tool": "acq_prog_times", "label": a.label, "lib": stamp, "N": N, "d": D, "P": P, "M_values": M_ACQ, "M_grad": M_GRAD,
           "instructions": int(prog.code.shape[0])}
    a_p, a_e = values["acq_prog"]()[0], values["acq_ei"]()[0]
    rec["max_abs_diff_prog_vs_ei"] = float(np.max(np.abs(a_p - a_e)))
    for group in (values, grads):
        ts = {k: [] for k in group}
        for k, f in group.items():
            f()
            f()
        for _ in range(a.reps):
            for k, f in group.items():
                ts[k].append(ms(f))
        for k in group:
            rec[k] = stats(ts[k])
    cand.close()
    for g in gps:
        g.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
