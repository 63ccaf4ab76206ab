"""What an interpreted Gram / K* build costs: a DeviceKernel spelling Matérn-5/2 beside the built-in Matérn-5/2.

  python tools/kernel_program_times.py --label run1 --out profiles/kernel_program.jsonl
  BOSS_LIB_PATH=<the parent commit's library> python tools/kernel_program_times.py --label parent1 --out profiles/kernel_program.jsonl

One process, every figure p50 / min / max of --reps calls (20) after two warm-up calls, a host clock around the WHOLE Python call (it
ends synchronised); every variant in a loop of its own, because a program handle's 7 ms call between two built-in calls leaves the
caches cold for the built-in one (alternated call by call, the built-in acquisition at N = 4096 reads 0.53 ms, in its own loop 0.47 ms).
d = 8, N = 1024 and 4096:
(a) update:  boss_gp_update on a resident handle (Gram matrix, factorisation, solves, log-determinant);
(b) acq_ei:  boss_acq_ei over 8192 resident candidates, arg-max only.
A library without boss_kgp_create (the parent commit's, selected with BOSS_LIB_PATH) is measured on the built-in kernel alone."""
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
    lib = api.load_library()
    if api.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    has_prog = hasattr(lib, "boss_kgp_create")
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    d, M = 8, (512 if a.small else 8192)
    rec = dict(label=a.label, source_hash=stamp, library=os.path.basename(api.LIB_PATH), reps=a.reps, small=a.small, d=d, candidates=M,
               program_kernel=has_prog)
    prog = None
    if has_prog:
        from boss_jl_amd.kernel import DeviceKernel
        prog = DeviceKernel(matern52, d).program
        rec["instructions"] = int(prog.code.shape[0])
    rng = np.random.default_rng(0)
    lam, amp, sig = np.full(d, 0.5), 1.0, 0.05
    for N in ((256, 1100) if a.small else (1024, 4096)):
        X = rng.uniform(0, 1, (d, N))
        y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
        cand = api.Candidates(np.asfortranarray(rng.uniform(0, 1, (d, M))))
        gps = {"builtin": api.GP(X, y, "matern52")}
        if has_prog:
            gps["program"] = api.KernelGP(X, y, prog)
        best = float(y.max())
        upd = each({k: (lambda g=g: g.update(lam, amp, sig)) for k, g in gps.items()}, a.reps)
        acq = each({k: (lambda g=g: api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)) for k, g in gps.items()}, a.reps)
        rec[f"N{N}"] = dict(update=upd, acq_ei=acq)
        if has_prog:                                         # the two handles answer alike (a measurement of a wrong result is none)
            ab = api.acq_ei([[gps["builtin"]]], cand, [1.0], None, best)
            ak = api.acq_ei([[gps["program"]]], cand, [1.0], None, best)
            rec[f"N{N}"]["max_abs_acq_difference"] = float(np.abs(ab[0] - ak[0]).max())
        for g in gps.values():
            g.close()
        cand.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
