"""SequentialBatchAM over a NonstationaryGP: the device append (boss_ngp_append), the tracked candidates (boss_ngp_track_create +
boss_track_sync + boss_acq_ei_tracks) and a whole B.nonstationary_sequential_batch, against the paths they replace.

  python tools/ngp_append_times.py [--out profiles/ngp_append.jsonl] [--tag this]
  BOSS_LIB_PATH=<the parent commit's libbosship.so> python tools/ngp_append_times.py --tag parent --out ...

The comparison is against the parent commit's library (its boss_ngp_append downloads the data, builds a second handle and factorises
from scratch), built into a scratch file and run with this same script: BOSS_LIB_PATH selects it and --tag names the line.  A
library without the track entry points measures the old paths alone.

Shapes: d = 8, N = 1024 / 2048 / 4096 observations with the first appended row 37 rows below a 128 boundary (22 single appends stay
inside one block row and inside the storage), M = 8192 candidates.  Each shape runs in ONE child process under its own time limit (a
shape that hangs or faults ends alone and nothing is started after it); host clock around calls that return synchronised results;
p50 / min / max of --reps calls (default 20) after 2 warm-up calls:
  append       (a) GibbsGP.append of one observation
  track        (b) Track.sync + acq_ei_tracks after that append              (new library only)
  predict      (b) the old path: GibbsGP.predict + acq_ei_moments after that append
  batch        (c) B.nonstationary_sequential_batch, batch_size 8, S = 1, at N = 2048 (new library only); --batch-reps fits (default 5)
  batch_loop   (c) the brute-force loop: nonstationary_acq_ei_batch, slice mean, slice append per selection
One line per shape is printed and, with --out, appended."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["N1024", "N2048", "N4096"]
D, M, BATCH = 8, 8192, 8


def stats(ts):
    return {"p50_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}


def child(shape, reps, batch_reps, tag):
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    from boss_jl_amd.problem import ExperimentData, LinFitness, best_so_far
    lib = api.load_library()
    has_tracks = hasattr(lib, "boss_ngp_track_create")
    N, d = int(shape[1:]), D
    N0 = N - 37
    rng = np.random.default_rng(0)
    Xall = rng.uniform(0, 1, (d, N0 + reps + 2))
    yall = np.sin(2 * np.pi * Xall).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(Xall.shape[1])
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
    lam_at = lambda Z: 0.3 + 0.4 * Z ** 2                                                  # noqa: E731  (d × points)
    amp_at = lambda Z: 1.0 + 0.4 * np.sin(3 * Z[0]) + 0.1 * Z[-1]                          # noqa: E731
    noi_at = lambda Z: 0.1 + 0.02 * Z[0]                                                   # noqa: E731
    lamS, ampS = lam_at(Xs), amp_at(Xs)
    best = float(yall[:N0].max())
    rec = {"shape": shape, "lib": tag, "rows": N0, "d": d, "candidates": M, "reps": reps, "tracks": has_tracks}

    g = api.GibbsGP(Xall[:, :N0], yall[:N0])
    g.update(lam_at(Xall[:, :N0]), amp_at(Xall[:, :N0]), noi_at(Xall[:, :N0]))
    cand = tr = None
    if has_tracks:
        cand = api.Candidates(Xs)
        tr = api.GibbsTrack(g, cand, lamS, ampS)
    t_app, t_trk, t_prd, paths = [], [], [], set()
    diff = 0.0
    for i in range(reps + 2):
        k = N0 + i
        x = Xall[:, k:k + 1]
        t = time.perf_counter()
        g.append(x, yall[k:k + 1], lam_at(x), amp_at(x), noi_at(x))
        t_app.append((time.perf_counter() - t) * 1e3)
        if has_tracks:
            paths.add(api._append_path(g))
            t = time.perf_counter()
            tr.sync()
            _, am_t, mx_t = api.acq_ei_tracks([[tr]], [1.0], None, best, want_acq=False)
            t_trk.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        mu, var = g.predict(Xs, lamS, ampS)
        _, am_p, mx_p = api.acq_ei_moments(mu[None, None, :], var[None, None, :], [1.0], None, best)
        t_prd.append((time.perf_counter() - t) * 1e3)
        if has_tracks:
            assert am_t == am_p, (am_t, am_p)
            diff = max(diff, abs(mx_t - mx_p))
    rec["append"] = stats(t_app[2:])
    rec["predict"] = stats(t_prd[2:])
    if has_tracks:
        rec["track"] = stats(t_trk[2:])
        rec["append_paths"] = sorted(paths)
        rec["max_abs_diff_acq_max"] = diff
        tr.close()
        cand.close()
    g.close()

    if N == 2048:
        f_lam = lambda Z: lam_at(Z).T                                                      # noqa: E731  (points × d)
        f_amp = lambda Z: amp_at(Z)                                                        # noqa: E731
        f_noi = lambda Z: noi_at(Z)                                                        # noqa: E731
        for f in (f_lam, f_amp, f_noi):
            f.vectorized = True
        model = B.HipNonstationaryGP([f_lam], [f_amp], [f_noi])
        data = ExperimentData(Xall[:, :N0], yall[None, :N0])

        def tracked(posts):
            return B.nonstationary_sequential_batch(posts, Xs, BATCH, [1.0], None, data.Y)

        def loop(posts):
            Y, xs = data.Y.copy(), []
            for _ in range(BATCH):
                b = best_so_far(LinFitness([1.0]), Y, [np.inf])
                _, am, _ = B.nonstationary_acq_ei_batch(posts, Xs, [1.0], None, b)
                x = Xs[:, am].copy()
                yh = np.array([np.mean([row[i].mean_and_var(x)[0] for row in posts]) for i in range(Y.shape[0])])
                for row in posts:
                    for i, p in enumerate(row):
                        p.append(x, yh[i])
                Y = np.concatenate([Y, yh[:, None]], axis=1)
                xs.append(x)
            return np.stack(xs, axis=1)
        sel = {}
        for name, call in (("batch", tracked), ("batch_loop", loop)):
            if name == "batch" and not has_tracks:
                continue
            ts = []
            for i in range(batch_reps + 1):                     # one warm-up
                posts = [model.model_posterior(data)]
                t = time.perf_counter()
                sel[name] = call(posts)
                ts.append((time.perf_counter() - t) * 1e3)
                for p in posts[0]:
                    p.close()
            rec[name] = stats(ts[1:])
        if "batch" in sel:
            rec["batch_selections_equal"] = bool(np.array_equal(sel["batch"], sel["batch_loop"]))
    print("TIMES " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="this")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch-reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--shape-timeout", type=int, default=240)
    ap.add_argument("--child", default=None)                     # shape (internal)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.batch_reps, a.tag)
        return 0
    for shape in a.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--batch-reps",
                                str(a.batch_reps), "--tag", a.tag], capture_output=True, text=True, timeout=a.shape_timeout)
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
