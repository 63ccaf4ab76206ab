"""What the batched program-kernel calls save: S hyper-parameter sets of a DeviceKernel spelling Matérn-5/2, d = 8.

  python tools/kernel_program_batch_times.py --N 1024 --S 64 --label this-run1 --out profiles/kernel_program_batch.jsonl
  BOSS_LIB_PATH=<the parent commit's library> python tools/kernel_program_batch_times.py --N 1024 --S 64 --label parent-run1 --out ...

One process per shape; every figure p50 / min / max of --reps calls (20) after two warm-up calls, a host clock around the whole Python
call (each ends synchronised), every variant in a loop of its own.  Per shape:
(a) loglike:  boss_kgp_loglike_batch for S sets           against  S boss_gp_update calls on one resident handle;
(b) fit:      boss_kgp_fit_batch, handles freed            against  boss_kgp_create + boss_gp_update per set, handles freed;
(c) acq_ei:   boss_acq_ei over S members, 8192 resident candidates, arg-max only — one set of launches with this library, member by
              member with a library that has no boss_kgp_fit_batch (the parent commit's: its handles are create + update ones).
The `loop` variants are what the Python layer ran before; a library without the batched entry points (selected with BOSS_LIB_PATH)
is measured on them alone.  Every line carries the source hash of the library it timed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    return dict(p50_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), calls=len(ts))


def timed(call, reps):
    for _ in range(2):
        call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return stats(ts)


def matern52(u, v):
    r2 = ((u - v) ** 2).sum()
    s = np.sqrt(5.0 * r2)
    return (1 + s + 5.0 / 3.0 * r2) * np.exp(-s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--S", type=int, default=8)
    ap.add_argument("--candidates", type=int, default=8192)
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from boss_jl_amd import api
    from boss_jl_amd.kernel import DeviceKernel
    lib = api.load_library()
    if api.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    batched = hasattr(lib, "boss_kgp_fit_batch")
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    d, N, S, M = 8, a.N, a.S, a.candidates
    prog = DeviceKernel(matern52, d).program
    rec = dict(label=a.label, source_hash=stamp, library=os.path.basename(api.LIB_PATH), reps=a.reps, d=d, N=N, S=S, candidates=M,
               batched_entry_points=batched, instructions=int(prog.code.shape[0]))
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    k = np.arange(S)
    lam = np.full((d, S), 0.5) * (1.0 + 0.3 * k / max(S, 1))[None, :]
    amp, sig = 1.0 + 0.2 * k / max(S, 1), np.full(S, 0.05)
    best = float(y.max())
    cand = api.Candidates(np.asfortranarray(rng.uniform(0, 1, (d, M))))

    one = api.KernelGP(X, y, prog)

    def loglike_loop():
        return np.array([one.update(lam[:, s], amp[s], sig[s]) for s in range(S)])

    def fit_loop(keep=False):
        gps = []
        for s in range(S):
            g = api.KernelGP(X, y, prog)
            g.update(lam[:, s], amp[s], sig[s])
            gps.append(g)
        if keep:
            return gps
        for g in gps:
            g.close()

    def fit_batched(keep=False):
        gps, _, _ = api.kgp_fit_batch(X, y, prog, lam, amp, sig)
        if keep:
            return gps
        for g in gps:
            g.close()

    rec["loglike"] = dict(loop=timed(loglike_loop, a.reps))
    rec["fit"] = dict(loop=timed(fit_loop, a.reps))
    want = loglike_loop()
    if batched:
        rec["loglike"]["batched"] = timed(lambda: api.kgp_loglike_batch(X, y, prog, lam, amp, sig), a.reps)
        rec["fit"]["batched"] = timed(fit_batched, a.reps)
        ll, st = api.kgp_loglike_batch(X, y, prog, lam, amp, sig)     # (a measurement of a wrong result is none)
        rec["loglike"]["batched_equals_loop"] = bool(np.array_equal(ll, want) and not st.any())
    one.close()
    # the averaged acquisition over the S posteriors: members of one fit with this library (set launches), create + update handles
    # with a library that has no batched fit (member by member)
    gps = fit_batched(True) if batched else fit_loop(True)
    rows = [[g] for g in gps]
    key = "set" if batched else "loop"
    rec["acq_ei"] = {key: timed(lambda: api.acq_ei(rows, cand, [1.0], None, best, want_acq=False), a.reps)}
    if batched:
        before = api._set_launches()[0]
        _, am, mx = api.acq_ei(rows, cand, [1.0], None, best, want_acq=False)
        rec["acq_ei"]["set_launches_per_call"] = int(api._set_launches()[0] - before)
        rec["acq_ei"]["argmax"], rec["acq_ei"]["max"] = int(am), float(mx)
    else:
        _, am, mx = api.acq_ei(rows, cand, [1.0], None, best, want_acq=False)
        rec["acq_ei"]["argmax"], rec["acq_ei"]["max"] = int(am), float(mx)
    for g in gps:
        g.close()
    cand.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
