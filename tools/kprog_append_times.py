"""SequentialBatchAM over a program kernel: the appended observation (boss_gp_append on a boss_kgp_set_sequential handle) and the
tracked candidates (boss_track_create + boss_track_sync + boss_acq_ei_tracks), beside the only route a library without the switch
has — a new handle of N + 1 points plus an update, and a fresh prediction of the candidates — and beside the built-in kernel.

  python tools/kprog_append_times.py [--out profiles/kprog_append.jsonl] [--tag this]

Shape: a Matérn-5/2 spelled as a program (31 instructions) and the built-in Matérn-5/2, d = 8, N = 4096 observations with the first
appended row 37 rows below the end of the storage (every append stays inside one block row and inside the storage), M = 8192
candidates.  Each kernel runs in ONE child process under its own time limit (a child that hangs or faults ends alone and nothing is
started after it); host clock around calls that return synchronised results; p50 / min / max of --reps calls (default 20) after 2
warm-up calls:
  append_first   one observation right after an update (block rows, route 1); every call follows a fresh update
  append_next    one observation from the second on (rank-one append on the resident inverse factors, route 3)
  refit          the route without the switch: a new handle over the N + 1 points plus update
  track          Track.sync + acq_ei_tracks after an append
  predict        the route without tracks: predict + acq_ei_moments after that append
One line per kernel is printed and, with --out, appended."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["program", "builtin"]
D, N, M = 8, 4096, 8192


def matern52(u, v):
    r2 = sum((u[k] - v[k]) ** 2 for k in range(len(u)))
    s = np.sqrt(5.0 * r2)
    return (1 + s + 5.0 / 3.0 * r2) * np.exp(-s)


def stats(ts):
    return {"p50_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def child(kind, reps, tag):
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    api.load_library()
    d, N0 = D, N - 37
    rng = np.random.default_rng(0)
    Xall = rng.uniform(0, 1, (d, N0 + reps + 4))
    yall = np.sin(2 * np.pi * Xall).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(Xall.shape[1])
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
    lam, amp, sig = np.linspace(0.4, 0.6, d), 1.0, 0.05
    best = float(yall[:N0].max())
    prog = B.DeviceKernel(matern52, d, sequential=True).program if kind == "program" else None
    rec = {"kernel": kind, "lib": tag, "rows": N0, "d": d, "candidates": M, "reps": reps}
    if prog is not None:
        rec["instructions"] = int(prog.code.shape[0])

    def handle(n):
        if prog is not None:
            return api.KernelGP(Xall[:, :n], yall[:n], prog, sequential=True)
        return api.GP(Xall[:, :n], yall[:n], "matern52")

    # (a) the first append after an update
    g = handle(N0)
    t_first, paths = [], set()
    for i in range(reps + 2):
        g.update(lam, amp, sig)
        k = N0 + i
        t = time.perf_counter()
        g.append(Xall[:, k:k + 1], yall[k:k + 1])
        t_first.append((time.perf_counter() - t) * 1e3)
        paths.add(api._append_path(g))
    rec["append_first"] = stats(t_first[2:])
    rec["append_first_paths"] = sorted(paths)
    g.close()

    # (b) the appends from the second on, the track beside a fresh prediction
    g = handle(N0)
    g.update(lam, amp, sig)
    cand = api.Candidates(Xs)
    tr = api.Track(g, cand)
    t_next, t_trk, t_prd, paths = [], [], [], set()
    diff = 0.0
    for i in range(reps + 3):
        k = N0 + i
        t = time.perf_counter()
        g.append(Xall[:, k:k + 1], yall[k:k + 1])
        t_next.append((time.perf_counter() - t) * 1e3)
        if i >= 1:
            paths.add(api._append_path(g))
        t = time.perf_counter()
        tr.sync()
        _, am_t, mx_t = api.acq_ei_tracks([[tr]], [1.0], None, best, want_acq=False)
        t_trk.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        mu, var = g.predict(Xs)
        _, am_p, mx_p = api.acq_ei_moments(mu[None, None, :], var[None, None, :], [1.0], None, best)
        t_prd.append((time.perf_counter() - t) * 1e3)
        assert am_t == am_p, (am_t, am_p)
        diff = max(diff, abs(mx_t - mx_p))
    rec["append_next"] = stats(t_next[3:])
    rec["append_next_paths"] = sorted(paths)
    rec["track"] = stats(t_trk[3:])
    rec["predict"] = stats(t_prd[3:])
    rec["max_abs_diff_acq_max"] = diff
    tr.close()
    cand.close()
    g.close()

    # (c) the route without the switch: a new handle of N0 + 1 points plus update
    t_refit = []
    for i in range(reps + 2):
        t = time.perf_counter()
        h = handle(N0 + 1)
        h.update(lam, amp, sig)
        t_refit.append((time.perf_counter() - t) * 1e3)
        h.close()
    rec["refit"] = stats(t_refit[2:])
    rec["append_p50_below_refit_min"] = bool(rec["append_first"]["p50_ms"] < rec["refit"]["min_ms"] and
                                             rec["append_next"]["p50_ms"] < rec["refit"]["min_ms"])
    print("TIMES " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--kind-timeout", type=int, default=240)
    ap.add_argument("--child", default=None)                     # kernel kind (internal)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.tag)
        return 0
    for kind in a.kinds.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--reps", str(a.reps), "--tag", a.tag],
                               capture_output=True, text=True, timeout=a.kind_timeout)
        except subprocess.TimeoutExpired:
            print(f"[times] {kind}: time limit of {a.kind_timeout} s reached; stopping", flush=True)
            return 1
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("TIMES ")), None)
        if r.returncode != 0 or line is None:                    # a fault or an error: nothing more is started on the device
            print(f"[times] {kind}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}", flush=True)
            return 1
        print(line[6:], flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line[6:] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
