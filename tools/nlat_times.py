"""Resident latent models (HipNonstationaryGP(resident_latents=True): boss_nlat_* and the _lat calls) against the closure path.

  python tools/nlat_times.py [--out profiles/nlat.jsonl]

Shape: d = 8; every λ_l(x) is a HipParametrizedGP posterior with a LogNormal target, α(x) one with softplus on a Normal target, all
on the N data points (N = 1024 / 2048); M = 224 starts and 1024 candidates.  Each shape runs in ONE child process under its own
time limit (a shape that hangs or faults ends alone and nothing is started after it); a host clock around calls that return
synchronised results; p50 / min / max of --reps calls (default 20) after 2 warm-up calls.
  slice/resident   mean_and_var_grad of one slice with resident latents (boss_ngp_predict_grad_lat)
  slice/floor      GibbsGP.predict_grad fed precomputed latent arrays: what the latent kernel adds lies between the two
  slice/closures   the same call on the closure path (central differences of the host closures), M = 224 only, --fd-reps calls
                   (default 3: one call is thousands of device calls, counted in "device_calls")
  set/resident     nonstationary_acq_ei_grad_batch over 64 members with resident latents (boss_ngp_acq_ei_grad_set_lat)
  set/arrays       ngp_acq_ei_grad_set fed precomputed arrays (the array route WITHOUT the time to produce its arrays)
  set/closures     the closure path over the 64 members, M = 224 only, --set-fd-reps calls (default 0 = not run)
The expectation is checked at EVERY shape and written as two flags: the resident route's p50 lies below the array route's fastest
call including the time that route spends producing its arrays.
  arrays_production_ms_per_member   what the closure path needs for one member's arrays: slice/closures' fastest call less slice/floor's
                   slowest, measured at M = 224 and the same N.  At M = 1024 the same figure is used, a lower bound there (the closure
                   path evaluates every candidate on its own, so 1024 candidates cost no less than 224).
  slice_resident_below_array_route  slice/resident p50 < slice/floor min + that production time
  set_resident_below_array_route    set/resident p50 < set/closures min where --set-fd-reps ran it ("set_comparison": "measured"), else
                   < set/arrays min + 64 × that production time ("extrapolated").  The set's closure path is one host loop over the
                   members (nonstationary_acq_ei_grad_batch), each member the slice's work, so one call of it is ≈ 64 × slice/closures,
                   minutes at these shapes: it is not run by default, and the flag then rests on the per-member figure measured above.
A shape run without its M = 224 shape before it (--shapes) has no production time and null flags.
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


def stats_of(ts):
    return {"p50_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": len(ts)}


def timed(call, reps, warm=2):
    ts = []
    for i in range(reps + warm):
        t = time.perf_counter()
        res = call()
        if i >= warm:
            ts.append((time.perf_counter() - t) * 1e3)
    return stats_of(ts), res


def child(shape, reps, fd_reps, set_fd_reps):
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    from boss_jl_amd.nonstationary import HipParametrizedGPParams
    from boss_jl_amd.problem import ExperimentData
    from scipy import stats
    N, M = (int(t[1:]) for t in shape.split("/"))
    d = D
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
    data = ExperimentData(X, y[None, :])
    pg_lam = B.HipParametrizedGP(np.full(d, 1.0), "matern52", stats.lognorm(0.2, scale=0.7), B.identity_act, 0.1)
    pg_amp = B.HipParametrizedGP(np.full(d, 1.0), "matern52", stats.norm(1.0, 0.3), B.softplus, 0.1)
    # one smooth factor for all latents' whitened outputs (the prior covariance at the data, as _params_sampler builds it)
    r = np.sqrt(((X[:, :, None] - X[:, None, :]) ** 2).sum(0))
    Lf = np.linalg.cholesky((1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r) + 0.01 * np.eye(N))
    mu0 = np.zeros(N)

    def model(resident):
        posts = [pg.model_posterior(HipParametrizedGPParams(X, mu0, Lf, rng.standard_normal(N), np.full(d, 1.0)))
                 for pg in [pg_lam] * d + [pg_amp]]
        m = B.HipNonstationaryGP([B.stack_latents(posts[:d])], [posts[d]], [B.constant_latent(0.1)], resident_latents=resident)
        return m, posts

    rec = {"shape": shape, "rows": N, "d": d, "candidates": M, "members": S, "reps": reps}
    # ---------------------------------------------------------------- one slice
    state = rng.bit_generator.state
    m_res, posts_res = model(True)
    sl = m_res.model_posterior_slice(data, 0)
    rec["slice/resident"], r1 = timed(lambda: sl.mean_and_var_grad(Xs), reps)
    lam, amp, _, dl, da = sl.latents.eval(Xs)
    rec["slice/floor"], r0 = timed(lambda: sl.gp.predict_grad(Xs, lam, amp, dl, da), reps)
    rec["latent_kernel_adds_ms"] = rec["slice/resident"]["p50_ms"] - rec["slice/floor"]["p50_ms"]
    assert all(np.array_equal(a, b) for a, b in zip(r0, r1))
    if M == 224 and fd_reps > 0:
        rng.bit_generator.state = state                         # the same latent draws
        m_cl, posts_cl = model(False)
        sc = m_cl.model_posterior_slice(data, 0)
        calls = [0]
        orig = api.GP.predict

        def counting(self, *a, **k):
            calls[0] += 1
            return orig(self, *a, **k)
        api.GP.predict = counting
        rec["slice/closures"], r2 = timed(lambda: sc.mean_and_var_grad(Xs), fd_reps, warm=1)
        api.GP.predict = orig
        rec["device_calls"] = calls[0] // (fd_reps + 1) + 1     # latent evaluations + the prediction itself
        rec["max_abs_diff_dmu_closures"] = float(np.abs(r2[2] - r1[2]).max())
        rec["resident_p50_below_closures_min"] = bool(rec["slice/resident"]["p50_ms"] < rec["slice/closures"]["min_ms"])
        sc.close()
        for p in posts_cl:
            p.close()
    sl.close()
    for p in posts_res:
        p.close()
    # ---------------------------------------------------------------- 64 members
    models, keep = [], []
    for _ in range(S):
        m, posts = model(True)
        models.append(m)
        keep.append(posts)
    posts = B.nonstationary_model_posterior_batch(models, data)
    for ps in keep:                                             # the resident objects hold snapshots: the latent handles may go
        for p in ps:
            p.close()
    best = float(y.max())
    rec["set/resident"], a1 = timed(lambda: B.nonstationary_acq_ei_grad_batch(posts, Xs, [1.0], None, best), reps)
    lamS, ampS = np.empty((d, M, S), order="F"), np.empty((M, S), order="F")
    Dl, Da = np.empty((d, d, M, S), order="F"), np.empty((d, M, S), order="F")
    t = time.perf_counter()
    for s in range(S):
        lamS[:, :, s], ampS[:, s], _, Dl[:, :, :, s], Da[:, :, s] = posts[s][0].latents.eval(Xs)
    rec["set/arrays_from_eval_ms"] = (time.perf_counter() - t) * 1e3
    gps = [[row[0].gp] for row in posts]
    rec["set/arrays"], a0 = timed(lambda: api.ngp_acq_ei_grad_set(gps, Xs, lamS, ampS, Dl, Da, [1.0], None, best), reps)
    assert all(np.array_equal(a, b) for a, b in zip(a0, a1))
    rec["set/closures"] = None
    for row in posts:
        for p in row:
            p.close()
    if M == 224 and set_fd_reps > 0:
        models, keep = [], []
        for _ in range(S):
            m, ps = model(False)
            models.append(m)
            keep.append(ps)
        posts = B.nonstationary_model_posterior_batch(models, data)
        rec["set/closures"], _ = timed(lambda: B.nonstationary_acq_ei_grad_batch(posts, Xs, [1.0], None, best), set_fd_reps, warm=0)
        for row in posts:
            for p in row:
                p.close()
        for ps in keep:
            for p in ps:
                p.close()
    print("TIMES " + json.dumps(rec), flush=True)


def compare(rec, production_ms):
    """The expectation, checked at every shape: the resident route's p50 lies below the array route's fastest call INCLUDING the time
    that route spends producing its arrays.  production_ms: what the closure path needed for ONE member's arrays at 224 starts and
    this N (slice/closures' fastest call less slice/floor's slowest); None when that shape was not run before this one."""
    rec["arrays_production_ms_per_member"] = production_ms
    rec["slice_resident_below_array_route"] = rec["set_resident_below_array_route"] = None
    rec["set_comparison"] = None
    if production_ms is None:
        return
    rec["slice_resident_below_array_route"] = bool(rec["slice/resident"]["p50_ms"] < rec["slice/floor"]["min_ms"] + production_ms)
    if rec.get("set/closures"):
        rec["set_comparison"] = "measured"
        rec["set_resident_below_array_route"] = bool(rec["set/resident"]["p50_ms"] < rec["set/closures"]["min_ms"])
    else:
        rec["set_comparison"] = "extrapolated"
        rec["set_resident_below_array_route"] = bool(rec["set/resident"]["p50_ms"] < rec["set/arrays"]["min_ms"] + rec["members"] * production_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fd-reps", type=int, default=3)
    ap.add_argument("--set-fd-reps", type=int, default=0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--shape-timeout", type=int, default=400)
    ap.add_argument("--child", default=None)                     # shape (internal)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.fd_reps, a.set_fd_reps)
        return 0
    production = {}                                              # rows -> ms the closure path needs for one member's arrays at 224 starts
    for shape in a.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps), "--fd-reps",
                                str(a.fd_reps), "--set-fd-reps", str(a.set_fd_reps)], capture_output=True, text=True, timeout=a.shape_timeout)
        except subprocess.TimeoutExpired:
            print(f"[times] {shape}: time limit of {a.shape_timeout} s reached; stopping", flush=True)
            return 1
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("TIMES ")), None)
        if r.returncode != 0 or line is None:                    # a fault or an error: nothing more is started on the device
            print(f"[times] {shape}: exit {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}", flush=True)
            return 1
        rec = json.loads(line[6:])
        if rec.get("slice/closures"):
            production[rec["rows"]] = rec["slice/closures"]["min_ms"] - rec["slice/floor"]["max_ms"]
        compare(rec, production.get(rec["rows"]))
        out = json.dumps(rec)
        print(out, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(out + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
