"""boss_ngp_acq_ei_grad_set (acquisition value and gradient of a nonstationary model averaged over the S samples of a BI fit, one
call) against the loop that is the only other public path: per member GibbsGP.predict_grad, per sample acq_ei_grad_moments, host mean.

  python tools/ngp_grad_set_times.py [--out profiles/ngp_grad_set.jsonl]

Shapes: 64 members of one ngp_fit_batch (one output), d = 8, N = 1024 and 2048, at M = 224 and 1024 candidates, every member with its
own latent values and Jacobians at the candidates.  Each shape runs in ONE child process under its own time limit (a shape that hangs
or faults ends alone and nothing is started after it) and measures, with a host clock around calls that return synchronised results:
  set         one ngp_acq_ei_grad_set call                     p50 / min / max of --reps calls (default 20) after 2 warm-up calls
  loop        the member-by-member path above                  the same
  first/set   the FIRST set call after a fit (it also builds the transposed factors and a = L⁻ᵀz): --first-reps refits (default 3)
  first/loop  the same for the loop
One line per shape is printed and, with --out, appended."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [f"N{N}/M{M}" for N in (1024, 2048) for M in (224, 1024)]
S, D = 64, 8


def child(shape, reps, first_reps):
    sys.path.insert(0, ROOT)
    from boss_jl_amd import api
    N, M = (int(t[1:]) for t in shape.split("/"))
    d = D
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
    sl, sa = rng.uniform(0.8, 1.4, S), rng.uniform(0.8, 1.3, S)
    lam_at = lambda Z, s: sl[s] * (0.3 + 0.4 * Z ** 2)                                     # noqa: E731  (d × points)
    amp_at = lambda Z, s: sa[s] * (1.0 + 0.4 * np.sin(3 * Z[0]) + 0.1 * Z[-1])             # noqa: E731
    lamX = np.asfortranarray(np.stack([lam_at(X, s) for s in range(S)], axis=2))
    ampX = np.asfortranarray(np.stack([amp_at(X, s) for s in range(S)], axis=1))
    noiX = np.asfortranarray(np.repeat((0.05 + 0.02 * X[0])[:, None], S, axis=1))
    lamS = np.asfortranarray(np.stack([lam_at(Xs, s) for s in range(S)], axis=2))
    ampS = np.asfortranarray(np.stack([amp_at(Xs, s) for s in range(S)], axis=1))
    Dl = np.zeros((d, d, M, S), order="F")
    Da = np.zeros((d, M, S), order="F")
    for s in range(S):
        for m in range(d):
            Dl[m, m, :, s] = sl[s] * 0.8 * Xs[m]
        Da[0, :, s] += sa[s] * 1.2 * np.cos(3 * Xs[0])
        Da[-1, :, s] += sa[s] * 0.1
    best = float(y.max())

    def fit():
        gps, _, st = api.ngp_fit_batch(X, y, lamX, ampX, noiX)
        assert not st.any()
        return gps

    def call_set(gps):
        return api.ngp_acq_ei_grad_set([[g] for g in gps], Xs, lamS, ampS, Dl, Da, [1.0], None, best)

    def call_loop(gps):
        acc, gacc = 0.0, 0.0
        for s, g in enumerate(gps):
            mu, var, dmu, dvar = g.predict_grad(Xs, lamS[:, :, s], ampS[:, s], Dl[:, :, :, s], Da[:, :, s])
            a, gr = api.acq_ei_grad_moments(mu[None], var[None], dmu[None], dvar[None], [1.0], None, best)
            acc, gacc = acc + a, gacc + gr
        return acc / S, gacc / S

    def timed(call, gps):
        t = time.perf_counter()
        res = call(gps)
        return (time.perf_counter() - t) * 1e3, res
    rec = {"shape": shape, "members": S, "rows": N, "d": d, "candidates": M, "reps": reps, "first_reps": first_reps}
    before = api._set_grad_launches()
    results = {}
    for name, call in (("set", call_set), ("loop", call_loop)):
        first = []
        for _ in range(first_reps):
            gps = fit()
            first.append(timed(call, gps)[0])
            if len(first) < first_reps:
                for g in gps:
                    g.close()
        ts = []
        for i in range(reps + 2):                                # two warm-up calls on the last fit
            dt, res = timed(call, gps)
            if i >= 2:
                ts.append(dt)
        results[name] = res
        for g in gps:
            g.close()
        rec[name] = {"p50_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}
        rec["first/" + name] = {"p50_ms": float(np.median(first)), "min_ms": float(min(first)), "max_ms": float(max(first))}
        if name == "set":
            rec["set_launches"] = bool(api._set_grad_launches() > before)
    assert np.all(np.isfinite(results["set"][0])) and np.all(np.isfinite(results["set"][1]))
    rec["max_abs_diff_acq"] = float(np.abs(results["set"][0] - results["loop"][0]).max())
    rec["max_abs_diff_grad"] = float(np.abs(results["set"][1] - results["loop"][1]).max())
    rec["set_p50_below_loop_min"] = bool(rec["set"]["p50_ms"] < rec["loop"]["min_ms"])
    print("TIMES " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--first-reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--shape-timeout", type=int, default=240)
    ap.add_argument("--child", default=None)                     # shape (internal)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.first_reps)
        return 0
    for shape in a.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--first-reps",
                                str(a.first_reps)], capture_output=True, text=True, timeout=a.shape_timeout)
        except subprocess.TimeoutExpired:
            print(f"[times] {shape}: time limit of {a.shape_timeout} s reached; stopping", flush=True)
            return 1
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("TIMES ")), None)
        if r.returncode != 0 or line is None:                    # a fault or an error: nothing more is started on the device
            print(f"[times] {shape}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}", flush=True)
            return 1
        print(line[6:], flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line[6:] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
