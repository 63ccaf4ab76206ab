"""Gradient-observation model: the device append (boss_ggp_append on block rows), the tracked candidates (boss_ggp_track_create +
boss_track_sync) and one B.gradient_sequential_batch selection, against the parent commit's rebuild-append.

  python tools/ggp_append_times.py [--out profiles/ggp_append.jsonl] [--tag this]
  BOSS_LIB_PATH=<the parent commit's libbosship.so> python tools/ggp_append_times.py --tag parent --out ...

The yardstick is the parent commit's library (its boss_ggp_append downloads the data, builds a second handle and factorises all
n(1+d) rows again), built into a scratch file and run with this same script: BOSS_LIB_PATH selects it and --tag names the line.  A
library without boss_ggp_reserve measures the append alone.

Shapes: d = 8 with n = 113 / 455 / 1024 points (1017 / 4095 / 9216 rows) and d = 3 with n = 256, M = 2048 candidates.  Each shape
runs in ONE child process under its own time limit (a shape that hangs or faults ends alone and nothing is started after it); host
clock around calls that return synchronised results; p50 / min / max of --reps calls (default 20) after 2 warm-up calls:
  update       boss_ggp_update on the (reserved) handle: what a full re-factorisation on the device costs at this shape (path 2)
  append       GradGP.append of one point (new library: after reserve + update, so nothing re-allocates)
  track        Track.sync after that append: the extension by the point's 1 + d rows        (new library only)
  predict      the path a track replaces: GradGP.predict at the same candidates after that append
  batch        one B.gradient_sequential_batch selection (batch_size 1, S = 1: reserve, re-update, track, select, append)   (new only)
One line per shape is printed and, with --out, appended."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["d8n113", "d8n455", "d8n1024", "d3n256"]
M = 2048


def stats(ts):
    return {"p50_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def child(shape, reps, tag):
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    lib = api.load_library()
    new = hasattr(lib, "boss_ggp_reserve")
    d, n = (int(v) for v in shape[1:].split("n"))
    rng = np.random.default_rng(0)
    nt = n + reps + 2
    X = rng.uniform(0, 1, (d, nt))
    w = np.linspace(1.0, 2.0, d)[:, None]
    y = np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(d)
    dY = 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(d)
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
    lam, hyp = np.linspace(0.4, 0.6, d), (1.1, 0.03, 0.07)
    rec = {"shape": shape, "lib": tag, "d": d, "points": n, "rows": n * (1 + d), "candidates": M, "reps": reps, "device_append": new}

    g = api.GradGP(X[:, :n], y[:n], dY[:, :n], "matern52")
    if new:
        g.update(lam, *hyp)
        g.reserve(points=nt)
    t_upd = []
    for _ in range(5):
        t = time.perf_counter()
        g.update(lam, *hyp)
        t_upd.append((time.perf_counter() - t) * 1e3)
    rec["update"] = stats(t_upd[1:])
    cand = tr = None
    if new:
        cand = api.Candidates(Xs)
        tr = api.GradTrack(g, cand)
    t_app, t_trk, t_prd, paths = [], [], [], set()
    diff = 0.0
    for i in range(reps + 2):
        k = n + i
        t = time.perf_counter()
        g.append(X[:, k:k + 1], y[k:k + 1], dY[:, k:k + 1])
        t_app.append((time.perf_counter() - t) * 1e3)
        if new:
            paths.add(api._append_path(g))
            t = time.perf_counter()
            tr.sync()
            t_trk.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        mu, var = g.predict(Xs)
        t_prd.append((time.perf_counter() - t) * 1e3)
        if new:
            mu_t, var_t = tr.moments()
            diff = max(diff, float(np.abs(mu_t - mu).max()), float(np.abs(var_t - var).max()))
    rec["append"] = stats(t_app[2:])
    rec["predict"] = stats(t_prd[2:])
    if new:
        rec["track"] = stats(t_trk[2:])
        rec["append_paths"] = sorted(paths)
        rec["max_abs_diff_track_predict"] = diff
        tr.close()
        cand.close()
    g.close()

    if new:
        prm = B.HipGradientGPParams(lam[:, None], [hyp[0]], [hyp[1]], [hyp[2]])
        model = B.HipGradientGaussianProcess([None], [None], [None], [None], kernel="matern52")
        data = B.GradientData(X[:, :n], y[None, :n], dY[None, :, :n])
        ts = []
        for _ in range(3):                                      # one warm-up
            post = model.model_posterior_slice(prm, data, 0)
            t = time.perf_counter()
            B.gradient_sequential_batch([[post]], Xs, 1, [1.0], None, data.Y)
            ts.append((time.perf_counter() - t) * 1e3)
            post.close()
        rec["batch"] = stats(ts[1:])
    print("TIMES " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--shape-timeout", type=int, default=240)
    ap.add_argument("--child", default=None)                     # shape (internal)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.tag)
        return 0
    for shape in a.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--tag", a.tag],
                               capture_output=True, text=True, timeout=a.shape_timeout)
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
