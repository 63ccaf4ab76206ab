"""What a DeviceMean saves: the Semiparametric mean traced into a device program beside the Python closure it replaces.

  python tools/device_mean_times.py --label run1 --out profiles/device_mean.jsonl

One process, every figure p50 / min / max of --reps calls (20) after two warm-up calls, a host clock around the WHOLE Python call (it
ends synchronised); the variants of one measurement alternate call by call.
(a) one HipGradientMAP round: the objective (log-posterior and all gradient groups) at 20 trial points, P = 2, N = 100, T = 3 —
    with a DeviceMean | the same closure with its exact parametric_jac | the mean held fixed (a constant mean, no θ group).  The last
    two are the paths this feature leaves as they are: the yardstick, re-measured in the same run.
(b) BASELINE config 4's shape, N = 2048, d = 6, P = 2, 8192 candidates, m_p(x) = θ_p0 + θ_p1..6ᵀx: the prior mean of all outputs at
    the candidates — host mean_values per output | one boss_mean_eval — and the whole HipBatchAM.maximize_acquisition both ways."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ts):
    return dict(p50_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), calls=len(ts))


def ms(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def alternate(calls, reps):
    """name -> stats, the calls taken in turn reps times after two warm-up rounds."""
    for _ in range(2):
        for c in calls.values():
            c()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, c in calls.items():
            ts[k].append(ms(c))
    return {k: stats(v) for k, v in ts.items()}


def mean3(x, th):
    return np.array([th[0] + th[1] * x[0] + np.cos(th[2] * x[1]), 0.5 * th[0] - th[1] * x[1] + np.cos(th[2] * x[0])])


def mean3_jac(x, th):
    return np.array([[1.0, x[0], -x[1] * np.sin(th[2] * x[1])], [0.5, -x[1], -x[0] * np.sin(th[2] * x[0])]])


def affine(x, th):
    return [th[0] + (th[1:7] * x).sum(), th[7] + (th[8:14] * x).sum()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="tiny shapes (a rehearsal of the script, not a measurement)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import boss_jl_amd as B
    from boss_jl_amd import api
    api.load_library()
    if api.device_count() < 1:
        raise SystemExit("no GPU: nothing to measure")
    side = api.LIB_PATH + ".srchash"
    stamp = open(side).read().strip()[:16] if os.path.exists(side) else "unknown"
    rng = np.random.default_rng(0)
    rec = dict(label=a.label, source_hash=stamp, reps=a.reps, small=a.small)

    # ---------------------------------------------------------------- (a) one HipGradientMAP round
    d, N, P, T, S = 2, (20 if a.small else 100), 2, 3, 20
    X = rng.uniform(0, 2, (d, N))
    truth = np.array([0.8, -0.6, 1.3])
    Y = np.stack([[mean3(X[:, j], truth)[i] for j in range(N)] for i in range(P)]) + 0.02 * rng.standard_normal((P, N))
    pri = dict(lengthscale_priors=[B.MvLogNormal([-0.5, -0.5], [0.3, 0.3])] * P, amplitude_priors=[B.LogNormal(-2.5, 0.3)] * P,
               noise_std_priors=[B.LogNormal(-3.5, 0.3)] * P)
    tp = [B.Normal(0.0, 2.0), B.Normal(0.0, 2.0), B.Normal(1.0, 1.0)]
    models = {"device_mean": B.HipGaussianProcess(parametric=B.DeviceMean(mean3, d, T, P), theta_priors=tp, **pri),
              "closure_exact_jac": B.HipGaussianProcess(parametric=mean3, parametric_jac=mean3_jac, theta_priors=tp, **pri),
              "mean_fixed": B.HipGaussianProcess(mean=[0.3, -0.1], **pri)}
    data = B.ExperimentData(X, Y)
    fitter = B.HipGradientMAP()
    sampler = models["device_mean"].params_sampler()
    trial = [sampler(rng) for _ in range(S)]
    calls = {}
    for name, model in models.items():
        obj = fitter._objective_semiparametric if model.parametric is not None else fitter._objective_batch
        calls[name] = (lambda obj=obj, model=model: obj(model, model.params_loglike(), data, trial))
    rec["map_round"] = dict(N=N, P=P, T=T, trial_points=S, **alternate(calls, a.reps))

    # ---------------------------------------------------------------- (b) config 4's shape
    d, N, P, M = 6, (128 if a.small else 2048), 2, (256 if a.small else 8192)
    X = rng.uniform(0, 1, (d, N))
    th = rng.standard_normal(14)
    Y = np.stack([np.sin(3 * X).sum(0) / np.sqrt(d), X[0] - X[1] + 0.2 * np.cos(4 * X[2])]) + 0.05 * rng.standard_normal((P, N))
    params = B.HipGPParams(np.full((d, P), 0.9), [1.0, 1.0], [0.05, 0.05], th)
    nopri = dict(lengthscale_priors=[None] * P, amplitude_priors=[None] * P, noise_std_priors=[None] * P, theta_priors=[None] * 14)
    Xs = np.asfortranarray(rng.uniform(0, 1, (d, M)))
    mk = lambda par: B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([0.7, -0.2])),   # noqa: E731
                                   B.HipGaussianProcess(parametric=par, **nopri), B.ExperimentData(X, Y), y_max=[np.inf, 0.8], params=params)
    p_dev, p_host = mk(B.DeviceMean(affine, d, 14, P)), mk(affine)
    rec["mean_at_candidates"] = dict(N=N, d=d, P=P, candidates=M, **alternate({
        "host_mean_values_all_outputs": lambda: [p_host.model.mean_values(Xs, params, i) for i in range(P)],
        "one_boss_mean_eval": lambda: p_dev.model.mean_values_all(Xs, params)}, a.reps))
    am = B.HipBatchAM(points=Xs)
    rec["maximize_acquisition"] = dict(N=N, d=d, P=P, candidates=M, **alternate({
        "closure": lambda: am.maximize_acquisition(p_host), "device_mean": lambda: am.maximize_acquisition(p_dev)}, a.reps))
    xa, va = am.maximize_acquisition(p_host)
    xb, vb = am.maximize_acquisition(p_dev)
    rec["maximize_acquisition"]["same_point"] = bool(np.array_equal(xa, xb))
    rec["maximize_acquisition"]["abs_value_difference"] = float(abs(va - vb))
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
