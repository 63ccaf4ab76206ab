"""boss_acq_ei_grad_set (acquisition value and gradient averaged over the S samples of a BI fit, one call) against the loop of
S boss_acq_ei_grad calls it replaces in HipGradientAM: ms per call.

  python tools/acq_grad_set_probe.py [--out profiles/acq_grad_set.jsonl]

Cases, 64 members each (one output): the plain model at N = 1024 and 2048, d = 8; the gradient model at n = 113 and 227, d = 8
(1017 and 2043 rows); M = 224 (one refinement round of the README's 224 starts) and 1024 candidates.
Per case four timed steps, each in a child process of its own under its own time limit (a step that hangs or faults ends alone and
nothing is started after it):
  grad/set    one boss_acq_ei_grad_set call over the members of one batched fit
  grad/loop   S boss_acq_ei_grad calls summed on the host (what HipGradientAM ran per iteration before the set call)
  prep/set    the same as grad/set, but the FIRST call after a fit: it also builds the transposed factors and a = L⁻ᵀz
  prep/loop   the same as grad/loop, first calls after a fit
Every step is warmed up (2 calls), then timed for --reps calls (default 20) with a host clock around work that ends in a
synchronisation (the calls return the results on the host); a line carries p50 / min / max.  The prep steps refit the members
before every timed call, outside the clock.  --members S runs fewer members; with BOSS_SET_GRAD_FILL=0 in the environment the
accumulation never splits the rows of a tile (the line then carries "fill").  The committed lines of both kinds are in
profiles/acq_grad_set.jsonl and profiles/acq_grad_set_split.jsonl."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"gp1024": ("gp", 1024, 8), "gp2048": ("gp", 2048, 8), "ggp1017": ("ggp", 113, 8), "ggp2043": ("ggp", 227, 8)}
CASES = [f"{k}/M{M}" for k in SHAPES for M in (224, 1024)]
STEPS = ("grad/set", "grad/loop", "prep/set", "prep/loop")
S = 64


def child(case, step, reps):
    sys.path.insert(0, ROOT)
    from boss_jl_amd import api
    shape, Mtxt = case.split("/")
    model, n, d = SHAPES[shape]
    M = int(Mtxt[1:])
    rng = np.random.default_rng(0)
    Xs = np.asfortranarray(rng.uniform(0, 1, (d, M)))
    X = rng.uniform(0, 1, (d, n))
    lam = rng.uniform(0.3, 1.5, (d, S))
    amp, sig, sgd = rng.uniform(0.5, 2.0, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
    if model == "ggp":
        w = rng.uniform(0.5, 2.0, d)
        y, dY = np.sin(X.T @ w), w[:, None] * np.cos(X.T @ w)[None, :]
        rows = n * (1 + d)

        def fit():
            gps, ll, st = api.ggp_fit_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
            assert not st.any()
            return gps
    else:
        y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(n)
        rows = n

        def fit():
            gps, ll, st = api.fit_batch(X, y, "matern52", lam, amp, sig)
            assert not st.any()
            return gps
    best = float(y.max())

    def call_set(gps):
        return api.acq_ei_grad_set([[g] for g in gps], Xs, [1.0], None, best)

    def call_loop(gps):
        acc, gacc = 0.0, 0.0
        for g in gps:
            a, gr = api.acq_ei_grad([g], Xs, [1.0], None, best)
            acc, gacc = acc + a, gacc + gr
        return acc / S, gacc / S
    call = call_set if step.endswith("/set") else call_loop
    before = api._set_grad_launches()
    ts = []
    gps = fit()
    for i in range(reps + 2):                                    # two warm-up calls
        if step.startswith("prep/") and i > 0:
            for g in gps:
                g.close()
            gps = fit()
        t = time.perf_counter()
        res = call(gps)
        dt = (time.perf_counter() - t) * 1e3
        if i >= 2:
            ts.append(dt)
    assert np.all(np.isfinite(res[0])) and np.all(np.isfinite(res[1]))
    took_set = api._set_grad_launches() > before
    for g in gps:
        g.close()
    rec = {"case": case, "step": step, "members": S, "rows": rows, "d": d, "candidates": M, "reps": len(ts), "p50_ms": float(np.median(ts)),
           "min_ms": float(min(ts)), "max_ms": float(max(ts)), "set_launches": bool(took_set)}
    if os.environ.get("BOSS_SET_GRAD_FILL"):
        rec["fill"] = int(os.environ["BOSS_SET_GRAD_FILL"])
    print("PROBE " + json.dumps(rec), flush=True)


def main():
    global S
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--members", type=int, default=S)            # fewer members: the accumulation splits the rows of a tile
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default=None)                     # case:step (internal)
    a = ap.parse_args()
    S = a.members
    if a.child:
        case, step = a.child.split(":")
        child(case, step, a.reps)
        return 0
    for case in a.cases.split(","):
        for step in a.steps.split(","):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{case}:{step}", "--reps", str(a.reps), "--members", str(a.members)],
                                   capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"[probe] {case} {step}: time limit of {a.step_timeout} s reached; stopping", flush=True)
                return 1
            line = next((ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")), None)
            if r.returncode != 0 or line is None:                # a fault or an error: nothing more is started on the device
                print(f"[probe] {case} {step}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}", flush=True)
                return 1
            print(line[6:], flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line[6:] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
