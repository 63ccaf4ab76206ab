"""Fitted sets of the gradient-observation and the nonstationary model, and their set-wide prediction, against the per-handle loops
they replace: ms per call.

  python tools/model_fit_batch_probe.py [--out profiles/model_fit_batch.jsonl]

Cases (the shapes the README quotes for the likelihood batches): 64 sets of n = 113, d = 8 (1017 rows) and of n = 227, d = 8
(2043 rows) of the gradient model; 64 sets of N = 1024 and of N = 2048, d = 4, of the nonstationary model; 8192 candidates each.
Per case four timed steps, each in a child process of its own under its own time limit (a step that hangs or faults ends alone and
nothing is started after it):
  fit/batched    one boss_ggp_fit_batch / boss_ngp_fit_batch call, handles freed (the slab is reused by the next call)
  fit/loop       S × (create + update + free) — what model_posterior ran per sample before the batched calls
  predict/set    boss_acq_ei over the S members (gradient model) / boss_ngp_predict_set (nonstationary model)
  predict/loop   the same call with BOSS_NO_SET_PREDICT=1 (gradient model: S launch pairs inside boss_acq_ei) / S boss_ngp_predict calls
Every step is warmed up (2 calls), then timed for --reps calls (default 20) with a host clock around work that ends in a
synchronisation; a line carries p50 / min / max.  predict lines also carry the rate S·M·Np² flop / p50 and its fraction of the fp64
MFMA peak (78.6 TFLOP/s, the figure the README's other rows use; Np = rows padded to 256)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF = 78.6
CASES = {"ggp1017": ("ggp", 113, 8), "ggp2043": ("ggp", 227, 8), "ngp1024": ("ngp", 1024, 4), "ngp2048": ("ngp", 2048, 4)}
STEPS = ("fit/batched", "fit/loop", "predict/set", "predict/loop")
S, M = 64, 8192


def timed(call, reps):
    for _ in range(2):
        call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def child(case, step, reps):
    sys.path.insert(0, ROOT)
    from boss_jl_amd import api
    model, n, d = CASES[case]
    rng = np.random.default_rng(0)
    Xs = rng.uniform(0, 1, (d, M))
    if model == "ggp":
        X = rng.uniform(0, 1, (d, n))
        w = rng.uniform(0.5, 2.0, d)
        y, dY = np.sin(X.T @ w), w[:, None] * np.cos(X.T @ w)[None, :]
        lam = rng.uniform(0.3, 1.5, (d, S))
        amp, sig, sgd = rng.uniform(0.5, 2.0, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
        rows = n * (1 + d)

        def fit_batched():
            gps, ll, st = api.ggp_fit_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
            assert not st.any()
            return gps

        def fit_loop():
            gps = []
            for s in range(S):
                g = api.GradGP(X, y, dY, "matern52")
                g.update(lam[:, s], amp[s], sig[s], sgd[s])
                gps.append(g)
            return gps

        def predictor(gps):
            cand = api.Candidates(Xs)
            best = float(y.max())
            return lambda: api.acq_ei([[g] for g in gps], cand, [1.0], None, best, want_acq=False)
    else:
        X = rng.uniform(0, 1, (d, n))
        y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(n)
        c, a, nz = rng.uniform(0.7, 1.6, S), rng.uniform(0.6, 1.8, S), rng.uniform(1.0, 3.0, S)
        f_lam = lambda Z: 0.25 + 0.5 * Z ** 2 + 0.1 * np.arange(1, d + 1)[:, None]            # noqa: E731
        f_amp = lambda Z: 1.0 + 0.4 * np.sin(3 * Z[0])                                        # noqa: E731
        lam = np.asfortranarray(f_lam(X)[:, :, None] * c)
        amp = np.asfortranarray(f_amp(X)[:, None] * a)
        noi = np.asfortranarray((0.03 + 0.05 * X[-1] ** 2)[:, None] * nz)
        lam_s = np.asfortranarray(f_lam(Xs)[:, :, None] * c)
        amp_s = np.asfortranarray(f_amp(Xs)[:, None] * a)
        rows = n

        def fit_batched():
            gps, ll, st = api.ngp_fit_batch(X, y, lam, amp, noi)
            assert not st.any()
            return gps

        def fit_loop():
            gps = []
            for s in range(S):
                g = api.GibbsGP(X, y)
                g.update(lam[:, :, s], amp[:, s], noi[:, s])
                gps.append(g)
            return gps

        def predictor(gps):
            if step == "predict/set":
                return lambda: api.ngp_predict_set(gps, Xs, lam_s, amp_s)
            return lambda: [g.predict(Xs, lam_s[:, :, s], amp_s[:, s]) for s, g in enumerate(gps)]

    def free(gps):
        for g in gps:
            g.close()
    if step.startswith("fit/"):
        make = fit_batched if step == "fit/batched" else fit_loop
        ts = timed(lambda: free(make()), reps)
    else:
        gps = fit_batched()
        before = api._set_launches()[1]
        ts = timed(predictor(gps), reps)
        took_set = api._set_launches()[1] > before
        assert took_set == (step == "predict/set"), (step, took_set)
        free(gps)
    rec = {"case": case, "step": step, "sets": S, "rows": rows, "candidates": M, "reps": len(ts), "p50_ms": float(np.median(ts)),
           "min_ms": float(min(ts)), "max_ms": float(max(ts))}
    if step.startswith("predict/"):
        Np = -(-rows // 256) * 256
        rec["tflops"] = S * M * float(Np) ** 2 / (rec["p50_ms"] * 1e-3) / 1e12
        rec["frac_fp64_mfma_peak"] = rec["tflops"] / PEAK_TF
    print("PROBE " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default=None)                     # case:step (internal)
    a = ap.parse_args()
    if a.child:
        case, step = a.child.split(":")
        child(case, step, a.reps)
        return 0
    for case in a.cases.split(","):
        for step in STEPS:
            env = dict(os.environ)
            if step == "predict/loop":
                env["BOSS_NO_SET_PREDICT"] = "1"
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{case}:{step}", "--reps", str(a.reps)], env=env,
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
