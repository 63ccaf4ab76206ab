"""The nonstationary likelihood and gradient in whitened latent parameters (boss_nfit_loglike_grad) against the path without it.

  python tools/nfit_times.py [--out profiles/nfit.jsonl] [--shapes N1024/S8 ...] [--reps 20]

Shape: d = 8, all d + 2 latents GP latents on two shared factors (the lengthscale latents on one, amplitude and noise on the other),
S ∈ {8, 64} parameter sets, N ∈ {1024, 2048}.  Each shape runs in ONE child process under its own time limit (a shape that hangs or
faults ends alone and nothing is started after it); a host clock around calls that return synchronised results; first call, then
p50 / min / max of --reps calls after one more warm-up call.
  resident   api.NgpWhitened.loglike_grad: de-whitening, transform, likelihood, gradient and pull-back in one device call
  host       what a caller did before: numpy de-whitening (L θ per latent) and transform, api.ngp_loglike_grad_batch, numpy pull-back
The two triangular products read every factor once per pass.  Two floors are written, both at 6.3 TB/s (the bandwidth a streaming
kernel achieves on this part; 8 TB/s is the specification): "l_floor_full_ms" = 2 passes × factors × N²·8 bytes, and
"l_floor_tri_ms" = the same for the N(N+1)/2 entries of the triangle, which is all the products need to read.  They are floors of
the two products ALONE: the timed call also holds the S factorisations and gradient passes both routes share, so the p50 columns
cannot be held against them; that needs per-kernel times (boss_prof_*), which this tool does not take."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [f"N{N}/S{S}" for N in (1024, 2048) for S in (8, 64)]
D = 8


def stats_of(ts):
    return {"p50_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts)), "calls": len(ts)}


def timed(call, reps):
    t = time.perf_counter()
    call()
    first = (time.perf_counter() - t) * 1e3
    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(stats_of(ts), first_ms=first)


def child(shape, reps):
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    N, S = (int(t[1:]) for t in shape.split("/"))
    d = D
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    r = np.sqrt(((X[:, :, None] - X[:, None, :]) ** 2).sum(0))
    factors = [np.linalg.cholesky((1 + np.sqrt(3) * r / 0.8) * np.exp(-np.sqrt(3) * r / 0.8) + 0.01 * np.eye(N)),
               np.linalg.cholesky((1 + np.sqrt(5) * r + 5 * r * r / 3) * np.exp(-np.sqrt(5) * r) + 0.01 * np.eye(N))]
    # (narrow amplitude and noise targets: the kernel's (α_i + α_j)/2 prefactor is not positive definite for every amplitude function,
    # and at N = 2048 wider ones give matrices whose Cholesky fails — every set of this family is PD, "sets_ok" counts them)
    specs = [("lognormal", (np.log(0.7), 0.2), "identity", 0.0)] * d + [("normal", (1.0, 0.05), "softplus", 0.2), ("normal", (-1.5, 0.2), "exp", 0.0)]
    factor_of = [0] * d + [1, 1]
    mu = np.zeros((N, d + 2), order="F")
    theta = np.asfortranarray(0.5 * rng.standard_normal((N * (d + 2), S)))
    h = api.NgpWhitened(X, y, factors, factor_of, specs, mu)

    def resident():
        return h.loglike_grad(theta)

    def host():
        th = theta.reshape(d + 2, N, S)
        v, dv = np.empty((d + 2, N, S)), np.empty((d + 2, N, S))
        for q in range(d + 2):
            v[q], dv[q] = B.latent_transform(specs[q], factors[factor_of[q]] @ th[q] + mu[:, q:q + 1])
        ll, st, dl, da, dn, _ = api.ngp_loglike_grad_batch(X, y, np.asfortranarray(v[:d]), np.asfortranarray(v[d]), np.asfortranarray(v[d + 1]))
        cot = np.concatenate([dl, da[None], dn[None]])
        g = np.empty((d + 2, N, S))
        for q in range(d + 2):
            g[q] = factors[factor_of[q]].T @ (cot[q] * dv[q])
        return ll, st, g.reshape(-1, S)
    out = {"shape": shape, "N": N, "S": S, "d": d, "resident": timed(resident, reps), "host": timed(host, reps)}
    a, b = resident(), host()
    out["max_abs_grad_diff"] = float(np.abs(a[2] - b[2]).max())
    out["sets_ok"] = [int((a[1] == 0).sum()), int((b[1] == 0).sum())]
    out["max_abs_ll_diff"] = float(np.abs(a[0] - b[0]).max())
    out["l_floor_full_ms"] = 2 * len(factors) * N * N * 8 / 6.3e12 * 1e3
    out["l_floor_tri_ms"] = 2 * len(factors) * (N * (N + 1) // 2) * 8 / 6.3e12 * 1e3
    h.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", nargs="*", default=SHAPES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--child")
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps)
    for shape in a.shapes:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reps", str(a.reps)], capture_output=True, text=True,
                           timeout=a.limit)
        if r.returncode != 0:
            print(f"{shape}: exit status {r.returncode}; nothing further is started\n{r.stdout[-2000:]}{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
