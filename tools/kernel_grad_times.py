"""What the interpreted gradient kernels cost: a DeviceKernel(grad=True) spelling Matérn-5/2 beside the built-in Matérn-5/2.

  python tools/kernel_grad_times.py --label run1 --out profiles/kernel_grad.jsonl

One process, every figure p50 / min / max of --reps calls (20) after two warm-up calls, a host clock around the WHOLE Python call (it
ends synchronised); every variant in a loop of its own (tools/kernel_program_times.py says why).  d = 8:
(a) update_llgrad:  boss_gp_update + boss_gp_loglike_grad on a resident handle, N = 1024 and N = 4096;
(b) acq_ei_grad:    boss_acq_ei_grad at 224 and at 1024 candidates, N = 4096 (one iteration of a multistart ascent).
These are records, not pass/fail bars: the interpreter is VALU-bound where the built-in path is not."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    return dict(p50_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), calls=len(ts))


def each(calls, reps):
    out = {}
    for k, c in calls.items():
        for _ in range(2):
            c()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            c()
            ts.append((time.perf_counter() - t) * 1e3)
        out[k] = stats(ts)
    return out


def matern52(u, v):
    r2 = ((u - v) ** 2).sum()
    s = np.sqrt(5.0 * r2)
    return (1 + s + 5.0 / 3.0 * r2) * np.exp(-s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from boss_jl_amd import api
    from boss_jl_amd.kernel import DeviceKernel
    api.load_library()
    if api.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    d = 8
    prog = DeviceKernel(matern52, d, grad=True).program
    rec = dict(label=a.label, source_hash=stamp, reps=a.reps, small=a.small, d=d, instructions=int(prog.code.shape[0]))
    rng = np.random.default_rng(0)
    lam, amp, sig = np.full(d, 0.5), 1.0, 0.05

    def step(g):
        g.update(lam, amp, sig)
        return g.loglike_grad()

    sizes = (256, 1100) if a.small else (1024, 4096)
    for N in sizes:
        X = rng.uniform(0, 1, (d, N))
        y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
        gps = {"builtin": api.GP(X, y, "matern52"), "program": api.KernelGP(X, y, prog, grad=True)}
        row = dict(update_llgrad=each({k: (lambda g=g: step(g)) for k, g in gps.items()}, a.reps))
        gb, gk = step(gps["builtin"])[1], step(gps["program"])[1]
        row["max_abs_llgrad_difference"] = float(np.abs(gb - gk).max())       # (a measurement of a wrong result is none)
        if N == sizes[-1]:
            best = float(y.max())
            for M in ((32, 96) if a.small else (224, 1024)):
                Xs = np.asfortranarray(rng.uniform(0, 1, (d, M)))
                row[f"acq_ei_grad_M{M}"] = each({k: (lambda g=g: api.acq_ei_grad([g], Xs, [1.0], None, best)) for k, g in gps.items()}, a.reps)
                ab, ak = api.acq_ei_grad([gps["builtin"]], Xs, [1.0], None, best), api.acq_ei_grad([gps["program"]], Xs, [1.0], None, best)
                row[f"max_abs_dacq_difference_M{M}"] = float(np.abs(ab[1] - ak[1]).max())
        rec[f"N{N}"] = row
        for g in gps.values():
            g.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
