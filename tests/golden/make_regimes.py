"""Generates tests/golden/regimes.json and regimes_arrays.npy: 50-digit truths (oracle/mp_oracle.py) of the plain GP, the gradient-observation model and the
Gibbs model over a grid of hyper-parameter regimes, for tests/test_regimes_host.py and tests/test_gpu_regimes.py.  The layout, the
inputs of a case and the bars are those of tests/regimes_cases.py.  Run from the repository root (about ten minutes on 8 cores):

    python tests/golden/make_regimes.py [--jobs K]

Grids
  plain   a = (d, N, M) = (2, 40, 6):  3 kernels × λ/√d ∈ {0.01, 0.1, 0.5, 3, 30} × α ∈ {0.05, 1.2, 30} × σ ∈ {1e-3, 0.05, 2}   (135)
          b = (3, 136, 9):            3 kernels × λ/√d ∈ {0.01, 30} × σ ∈ {1e-3, 2} at α = 1.2, and λ/√d = 0.5, σ = 0.05 per kernel (15)
          candidate 0 lies on a training point, candidate 1 outside the data's hull; every third case carries a prior mean.
  grad    (d, n) = (2, 12), (2, 45):  3 kernels × λ/√d ∈ {0.05, 0.5, 5, 30} × σ ∈ {1e-3, 0.05} × σ_∂ ∈ {1e-2, 1} at α = 1.2            (96)
          no candidate on a training point (candidate 0 lies outside the hull).
  gibbs   N = 40, 136, d = 2:         geometric mean of λ(x) ∈ {0.05, 0.5, 5} × contrast of λ ∈ {1, 10, 100} × of α ∈ {1, 10} × of σ ∈ {1, 100}  (72)
          a case whose 50-digit Cholesky fails is dropped (the (α_i+α_j)/2 prefactor is not positive definite for every α(·)).

Asserted before anything is written: the fp64 oracle within 1/8 of the bar of every truth; at most a tenth of the Gibbs cases
dropped; at most a quarter of all (case, candidate) pairs removed by the variance-clip rule; the on-a-training-point candidate kept
wherever the var bar is <= 1e-9.  The worst oracle ratio err/(B·scale) per model and output goes into the header."""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import gp_oracle as O  # noqa: E402
from oracle import mp_oracle as MP  # noqa: E402
import regimes_cases as R  # noqa: E402

KID = {"matern32": 0, "matern52": 1, "sqexp": 2}


def _points(seed, d, N, M, on_point):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = rng.uniform(0, 1, (d, M))
    Xs[:, 0] = np.array([1.25, -0.2, 1.1])[:d]                 # outside the hull
    if on_point:
        Xs[:, 1] = Xs[:, 0]
        Xs[:, 0] = X[:, 7]                                     # on a training point
    return X, y, Xs


def datasets():
    out = {"plain": {}, "grad": {}, "gibbs": {}}
    for name, seed, d, N, M in (("a", 11, 2, 40, 6), ("b", 12, 3, 136, 9)):
        X, y, Xs = _points(seed, d, N, M, True)
        out["plain"][name] = {"X": X, "y": y, "Xs": Xs}
    for name, seed, n in (("n12", 21, 12), ("n45", 22, 45)):
        X, _, Xs = _points(seed, 2, n, 5, False)
        out["grad"][name] = {"X": X, "y": np.sin(2 * np.pi * X).sum(0) / np.sqrt(2), "dY": 2 * np.pi * np.cos(2 * np.pi * X) / np.sqrt(2), "Xs": Xs}
    for name, seed, N in (("n40", 47, 40), ("n136", 143, 136)):
        X, y, Xs = _points(seed, 2, N, 4, True)
        out["gibbs"][name] = {"X": X, "y": y, "Xs": Xs}
    return out


def grid():
    jobs = []
    k = 0
    for kern in R.KERNELS:
        for lr in (0.01, 0.1, 0.5, 3.0, 30.0):
            for amp in (0.05, 1.2, 30.0):
                for sig in (1e-3, 0.05, 2.0):
                    jobs.append(("plain", dict(data="a", kernel=kern, lam_rel=lr, amp=amp, sig=sig, mean=(k % 3 == 0))))
                    k += 1
    for kern in R.KERNELS:
        for lr, sig in ((0.01, 1e-3), (0.01, 2.0), (30.0, 1e-3), (30.0, 2.0), (0.5, 0.05)):
            jobs.append(("plain", dict(data="b", kernel=kern, lam_rel=lr, amp=1.2, sig=sig, mean=(k % 3 == 0))))
            k += 1
    for data in ("n12", "n45"):
        for kern in R.KERNELS:
            for lr in (0.05, 0.5, 5.0, 30.0):
                for sig in (1e-3, 0.05):
                    for gsig in (1e-2, 1.0):
                        jobs.append(("grad", dict(data=data, kernel=kern, lam_rel=lr, amp=1.2, sig=sig, gsig=gsig)))
    for data in ("n40", "n136"):
        for gm in (0.05, 0.5, 5.0):
            for cl in (1, 10, 100):
                for ca in (1, 10):
                    for cs in (1, 100):
                        jobs.append(("gibbs", dict(data=data, gm=gm, clam=cl, camp=ca, csig=cs)))
    ds = datasets()
    for model, c in jobs:
        c.update(R.derived(model, ds[model][c["data"]], c))          # name, rows, amp2
    return jobs


def truth(job):
    """One case's 50-digit truths (a worker process); None where the Gibbs matrix is not positive definite."""
    model, c = job
    fx = {m: {"datasets": ds} for m, ds in datasets().items()}
    if model == "plain":
        X, y, Xs, lam, amp, sig, mX, ms = R.plain_inputs(fx, c)
        t = MP.plain_truth(X.tolist(), y, KID[c["kernel"]], lam, amp, sig, Xs.tolist(), mX, ms)
    elif model == "grad":
        X, y, dY, Xs, lam, amp, sig, gsig = R.grad_inputs(fx, c)
        t = MP.grad_obs_truth(X.tolist(), y, dY.tolist(), KID[c["kernel"]], lam, amp, sig, gsig, Xs.tolist())
    else:
        X, y, Xs, lam, amp, noi, lam_s, amp_s = R.gibbs_inputs(fx, c)
        try:
            t = MP.gibbs_truth(X.tolist(), y, lam.tolist(), amp, noi, Xs.tolist(), lam_s.tolist(), amp_s)
        except (ValueError, ZeroDivisionError):
            return model, c, None
        t.pop("dmean")
    return model, c, {k: np.asarray(v, dtype=np.float64) for k, v in t.items()}


def cost(job):
    model, c = job
    return {"plain": 1.0, "grad": 30.0, "gibbs": 2.0}[model] * c["rows"] ** 2


def main():
    nproc = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(8, os.cpu_count() or 1)
    jobs = grid()
    order = sorted(range(len(jobs)), key=lambda i: -cost(jobs[i]))
    with ProcessPoolExecutor(nproc) as pool:
        done = list(pool.map(truth, [jobs[i] for i in order], chunksize=1))
    results = [None] * len(jobs)
    for i, r in zip(order, done):
        results[i] = r
    ds = datasets()
    fx = {m: {"datasets": ds[m], "cases": []} for m in ds}
    dropped = []
    for model, c, t in results:
        if t is None:
            dropped.append(c["name"])
            continue
        c.update(t)
        c["logpdf"] = float(c["logpdf"])
        c["cond"] = float(f"{R.cond_of(O, model, fx, c):.6e}")
        fx[model]["cases"].append(c)
    n_gibbs = sum(1 for m, _, _ in results if m == "gibbs")
    print(f"gibbs cases dropped (50-digit Cholesky failed): {len(dropped)} of {n_gibbs}: {dropped}")
    assert 10 * len(dropped) <= n_gibbs, "more than a tenth of the Gibbs cases dropped: change α(·)"
    # the fp64 oracle within bar/8, and the worst ratios
    worst = {}
    for model in fx:
        for c in fx[model]["cases"]:
            r = R.check(c, R.oracle_outputs(O, model, fx, c), model, "oracle", frac=1.0 / 8)
            for k, v in r.items():
                worst.setdefault(model, {})[k] = max(worst.get(model, {}).get(k, 0.0), v)
    print("worst oracle err/(B·scale):", json.dumps(worst))
    # the variance-clip rule
    pairs = removed = 0
    for model in fx:
        for c in fx[model]["cases"]:
            keep = R.keep_mask(c)
            pairs += keep.size
            removed += int((~keep).sum())
            if model != "grad" and R.bar_var(c) <= 1e-9:
                assert keep[0], f"{c['name']}: the candidate on a training point is removed at var bar {R.bar_var(c):.3g}"
    print(f"candidates removed by the clip rule: {removed} of {pairs}")
    assert 4 * removed <= pairs, "more than a quarter of the (case, candidate) pairs removed"
    header = {"u": R.U, "bars": "see tests/regimes_cases.py", "gibbs_dropped": dropped, "clip_removed": [removed, pairs],
              "oracle_worst_ratio": {m: {k: float(f"{v:.3e}") for k, v in w.items()} for m, w in worst.items()}}

    # the arrays one after the other in one float64 vector; the rest as JSON, one case per line
    flat, at, lines = [], 0, ['{"header":' + json.dumps(header, separators=(",", ":"))]

    def put(entry, layout):
        nonlocal at
        out = {k: v for k, v in entry.items() if k not in dict(layout) and k not in ("name", "rows", "amp2")}
        out["at"] = at
        for k, shp in layout:
            assert np.shape(entry[k]) == shp, (k, np.shape(entry[k]), shp)
            flat.append(np.asarray(entry[k], dtype=np.float64).reshape(-1))
            at += flat[-1].size
        return json.dumps(out, separators=(",", ":"))

    for model in fx:
        sizes = {n: dict(d=D["X"].shape[0], N=D["X"].shape[1], M=D["Xs"].shape[1]) for n, D in fx[model]["datasets"].items()}
        dsets = [f'"{n}":' + put({**sizes[n], **D}, R.data_layout(model, **sizes[n])) for n, D in fx[model]["datasets"].items()]
        cases = [put(c, R.truth_layout(model, fx[model]["datasets"][c["data"]])) for c in fx[model]["cases"]]
        lines.append(f',"{model}":{{"datasets":{{' + ",".join(dsets) + '},"cases":[')
        lines += [ln + "," for ln in cases[:-1]] + [cases[-1] + "]}"]
    with open(R.PATH, "w") as f:
        f.write("\n".join(lines) + "}\n")
    np.save(R.ARRAYS, np.concatenate(flat))
    size = os.path.getsize(R.PATH) + os.path.getsize(R.ARRAYS)
    print("wrote", R.PATH, "and", R.ARRAYS, size, "bytes")
    assert size < 400000, "the fixture must stay below gp_golden.json's size"


if __name__ == "__main__":
    main()
