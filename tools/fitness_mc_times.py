"""What the Monte-Carlo EI of a nonlinear fitness costs on the device, beside the host path it replaces and the analytic EI.

  python tools/fitness_mc_times.py --label run1 --out profiles/fitness_mc.jsonl
  python tools/fitness_mc_times.py --label parent --only host --root <checkout of the parent commit> --out profiles/fitness_mc.jsonl

Setup: fitness cos(y0) + sin(y1), P = 2 outputs, N = 1024 observations, d = 8, K = 200 ε-samples, one posterior sample (MAP).
Measured, each with a host clock around the WHOLE Python call (it ends synchronised), after two warm-up calls:
  acquisition_values at 8192 candidates        DeviceFitness (boss_acq_ei_mc) | LinFitness (boss_acq_ei) | NonlinFitness (host path)
  HipGradientAM._value_and_grad at 224, 1024   DeviceFitness (boss_acq_ei_mc_grad) | LinFitness (boss_acq_ei_grad)
p50 / min / max of --reps calls (20); the host path takes seconds per call and gets --host-reps (3).  The device and LinFitness
calls alternate call by call.  `--only host` measures the host path alone, `--root` imports the package from another checkout
(the parent commit's, built there), so the host figure can be taken on code this change has not touched."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, N, D, K, M_ACQ, STARTS = 2, 1024, 8, 200, 8192, (224, 1024)


def stats(ts):
    return dict(p50_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), calls=len(ts))


def ms(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def fitness(y):
    return np.cos(y[0]) + np.sin(y[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="all", choices=("all", "device", "host"))
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import boss_jl_amd as B
    from boss_jl_amd import api
    from boss_jl_amd.maximizer import acquisition_values, posteriors_of
    api.load_library()
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (D, N))
    Y = np.stack([np.sin(3 * X).sum(0) / np.sqrt(D), X[0] - X[1] + 0.2 * np.cos(4 * X[2])]) + 0.05 * rng.standard_normal((P, N))
    mk = lambda fit: B.BossProblem(f=None, domain=B.Domain(bounds=(np.zeros(D), np.ones(D))), y_max=[np.inf, 0.8],            # noqa: E731
                                   acquisition=B.ExpectedImprovement(fit, eps_samples=K),
                                   model=B.HipGaussianProcess(lengthscale_priors=[None] * P, amplitude_priors=[None] * P,
                                                              noise_std_priors=[None] * P),
                                   data=B.ExperimentData(X, Y), params=B.HipGPParams(np.full((D, P), 0.9), [1.0, 1.0], [0.05, 0.05]))
    Xs = np.asfortranarray(rng.uniform(0, 1, (D, M_ACQ)))
    rec = dict(P=P, N=N, d=D, K=K, candidates=M_ACQ, label=a.label, source_hash=stamp, root=os.path.relpath(os.path.abspath(a.root), ROOT))
    runs = {}
    if a.only in ("all", "device"):
        p_dev, p_lin = mk(B.DeviceFitness(fitness, P)), mk(B.LinFitness([0.7, -0.2]))
        posts = posteriors_of(p_dev)
        am = B.HipGradientAM()
        pairs = {"acq_8192": (lambda: acquisition_values(p_dev, posts, Xs), lambda: acquisition_values(p_lin, posts, Xs))}
        for m in STARTS:
            X0 = np.asfortranarray(Xs[:, :m])
            pairs[f"grad_{m}"] = (lambda X0=X0: am._value_and_grad(p_dev, posts, X0), lambda X0=X0: am._value_and_grad(p_lin, posts, X0))
        for name, (dev, lin) in pairs.items():
            for _ in range(2):
                dev(), lin()
            td, tl = [], []
            for _ in range(a.reps):
                td.append(ms(dev))
                tl.append(ms(lin))
            runs[name + "_device_mc"], runs[name + "_lin_analytic"] = stats(td), stats(tl)
        for p in posts:
            p.close()
    if a.only in ("all", "host"):
        p_host = mk(B.NonlinFitness(fitness))
        posts = posteriors_of(p_host)
        call = lambda: acquisition_values(p_host, posts, Xs)                                                                  # noqa: E731
        runs["acq_8192_host_nonlin"] = stats([ms(call) for _ in range(a.host_reps)])
        for p in posts:
            p.close()
    rec.update(runs)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
