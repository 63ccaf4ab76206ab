"""Generates tests/golden/regimes_more.json and regimes_more_arrays.npy: further 50-digit truths (oracle/mp_oracle.py) over the regimes of
tests/golden/regimes.json, for tests/test_regimes_more_host.py and tests/test_gpu_regimes_more.py.  Datasets and the cases' parameters
are read from the first fixture (regimes_cases.load()), whose cases are referred to by name; nothing it holds is computed again.  The
layout, the inputs of a case and the bars are those of tests/regimes_cases.py.  Run from the repository root (about three minutes on 8
cores; the augmented Gram matrices of the gradient-observation model dominate):

    python tests/golden/make_regimes_more.py [--jobs K]

Added to the existing cases
  plain   cov[M][M]                         all 150 cases
  grad    dmu[d][M], dvar[d][M], cov[M][M]  all 96 cases
  gibbs   dmu, dvar, cov                    the cases the first fixture kept; the candidates' Jacobians are those of the log-linear
                                            latent fields in closed form (regimes_cases.gibbs_latent_jacobians)
New cases, model "kprog": program-kernel posteriors (logpdf, mu, var, dmu, dvar, llgrad[d+2]) on the plain datasets
  closures expo, ratquad, persq, dot1 of tests/kernel_program_cases.py, each traced once per dimension; the truth evaluates the traced
  program with the 50-digit interpreter (fitness_mc_cases.mp_eval)
  a = (2, 40, 6):   λ/√d ∈ {0.05, 0.5, 30} × (α, σ) ∈ {(1.2, 1e-3), (1.2, 0.05), (30, 1e-3), (0.05, 2), (1.2, 2)}                (60)
  b = (3, 136, 9):  (λ/√d, σ) ∈ {(0.05, 1e-3), (30, 1e-3), (0.5, 0.05)} at α = 1.2                                              (12)
  every third case carries the prior mean; expo leaves candidate 0 (on a training point: a cusp) out of dmu and dvar (NaN).
  (α, σ) = (1.2, 2) is there for the clip rule's cap: at σ = 1e-3 the smooth closures at λ/√d >= 0.5 and the finite-rank dot1 have
  posterior variances of 1e-8 … 1e-6 at cond(K) of 1e7 … 1e12, so the rule removes every candidate of those cases (they still pin
  logpdf and llgrad) — 114 of the 396 pairs without the fifth pair, more than the quarter allowed; with it 114 of 468.

The multiplier of a new quantity's bar stays at 8 (cov, and kprog's logpdf, mu, var) or 100 (gradients) where the fp64 oracle's worst
err/(B·scale) over the grid is at most an eighth of it, and is otherwise 8 × that worst ratio rounded up to a power of two
(regimes_cases.multiplier_of): chosen from the oracle alone, never from a device run.  Worst ratios and multipliers go into the header.

Asserted before anything is written: at most a tenth of the kprog cases dropped (50-digit Cholesky failed); the oracle within 1/8 of
every bar; at most a quarter of the kprog (case, candidate) pairs removed by the variance-clip rule; the on-a-training-point
candidate kept wherever the var bar is <= 1e-9; each of the two files below 400 000 bytes."""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor
from types import SimpleNamespace

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
CAP = 400000


def kprog_grid():
    """The declared kprog cases (parameters only), in the fixture's order."""
    out = []
    for closure in R.KPROG_CLOSURES:
        for lr in (0.05, 0.5, 30.0):
            for amp, sig in ((1.2, 1e-3), (1.2, 0.05), (30.0, 1e-3), (0.05, 2.0), (1.2, 2.0)):
                out.append(dict(data="a", closure=closure, lam_rel=lr, amp=amp, sig=sig, mean=(len(out) % 3 == 0)))
    for closure in R.KPROG_CLOSURES:
        for lr, sig in ((0.05, 1e-3), (30.0, 1e-3), (0.5, 0.05)):
            out.append(dict(data="b", closure=closure, lam_rel=lr, amp=1.2, sig=sig, mean=(len(out) % 3 == 0)))
    return out


def grid(fx):
    """[(model, case)]: every case of the first fixture, then the kprog cases with their derived entries."""
    jobs = [(model, c) for model in ("plain", "grad", "gibbs") for c in fx[model]["cases"]]
    for c in kprog_grid():
        c.update(R.kprog_derived(fx["plain"]["datasets"][c["data"]], c))
        jobs.append(("kprog", c))
    return jobs


def truth(job):
    """One case's further truths (a worker process); None where a kprog matrix is not positive definite at 50 digits."""
    model, c, prog = job
    fx = R.load()
    if model == "plain":
        X, _, Xs, lam, amp, sig, _, _ = R.plain_inputs(fx, c)
        t = {"cov": MP.plain_cov_truth(X.tolist(), KID[c["kernel"]], lam, amp, sig, Xs.tolist())}
    elif model == "grad":
        X, y, dY, Xs, lam, amp, sig, gsig = R.grad_inputs(fx, c)
        t = MP.grad_obs_pred_truth(X.tolist(), y, dY.tolist(), KID[c["kernel"]], lam, amp, sig, gsig, Xs.tolist())
    elif model == "gibbs":
        X, y, Xs, lam, amp, noi, lam_s, amp_s = R.gibbs_inputs(fx, c)
        dlam_s, damp_s = R.gibbs_latent_jacobians(Xs, c)
        t = MP.gibbs_pred_truth(X.tolist(), y, lam.tolist(), amp, noi, Xs.tolist(), lam_s.tolist(), amp_s, dlam_s.tolist(), damp_s.tolist())
    else:
        X, y, Xs, lam, amp, sig, mX, ms = R.plain_inputs(fx, c)
        try:
            t = MP.kprog_truth(R.mp_kernel(prog), X.tolist(), y, lam, amp, sig, Xs.tolist(), mX, ms, no_grad_at=R.no_grad_at(c))
        except (ValueError, ZeroDivisionError):
            return model, c["name"], None
    return model, c["name"], {k: np.asarray(v, dtype=np.float64) for k, v in t.items()}


def cost(job):
    model, c, _ = job
    return {"plain": 1.0, "grad": 30.0, "gibbs": 2.0, "kprog": 20.0}[model] * c["rows"] ** 2


def main():
    nproc = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(8, os.cpu_count() or 1)
    import __graft_entry__ as entry
    entry.build()
    import boss_jl_amd as B
    progs = R.kprog_programs(B)
    fx = R.load()
    # (the workers need the programs' instructions only, not the library's handles)
    plain_progs = {k: SimpleNamespace(consts=p.consts.copy(), code=p.code.copy(), out_id=p.out_id) for k, p in progs.items()}
    jobs = [(m, c, plain_progs[(c["closure"], fx["plain"]["datasets"][c["data"]]["X"].shape[0])] if m == "kprog" else None)
            for m, c in grid(fx)]
    order = sorted(range(len(jobs)), key=lambda i: -cost(jobs[i]))
    with ProcessPoolExecutor(nproc) as pool:
        done = list(pool.map(truth, [jobs[i] for i in order], chunksize=1))
    results = [None] * len(jobs)
    for i, r in zip(order, done):
        results[i] = r
    fxm = {m: [] for m in R.MODELS_MORE}
    dropped = []
    for (model, c, _), (_, name, t) in zip(jobs, results):
        assert name == c["name"]
        if t is None:
            dropped.append(name)
            continue
        c = dict(c)
        c.update(t)
        if model == "kprog":
            c["logpdf"] = float(c["logpdf"])
            X, y, Xs, lam, amp, sig, mX, ms = R.plain_inputs(fx, c)
            c["cond"] = float(f"{R.kprog_oracle(progs[(c['closure'], X.shape[0])], c, X, y, Xs, lam, amp, sig, mX, ms)[1]:.6e}")
        fxm[model].append(c)
    n_kprog = sum(1 for m, _, _ in jobs if m == "kprog")
    print(f"kprog cases dropped (50-digit Cholesky failed): {len(dropped)} of {n_kprog}: {dropped}")
    assert 10 * len(dropped) <= n_kprog, "more than a tenth of the kprog cases dropped"
    # the fp64 oracle's worst ratios, the multipliers they imply, and the oracle within an eighth of every bar
    worst = {}
    for model in R.MODELS_MORE:
        for c in fxm[model]:
            for got, keep in R.oracle_more(O, model, fx, c, progs=progs):
                for k, v in R.ratios(c, got, model, keep).items():
                    worst.setdefault(model, {})[k] = max(worst.get(model, {}).get(k, 0.0), v)
    print("worst oracle err/(B·scale):", json.dumps(worst))
    mult = {m: {k: R.multiplier_of(k, v) for k, v in w.items()} for m, w in worst.items()}
    print("multipliers:", json.dumps(mult))
    header = {"u": R.U, "bars": "see tests/regimes_cases.py", "kprog_dropped": dropped,
              "oracle_worst_ratio": {m: {k: float(f"{v:.3e}") for k, v in w.items()} for m, w in worst.items()}, "multiplier": mult}
    for model in R.MODELS_MORE:
        for c in fxm[model]:
            for got, keep in R.oracle_more(O, model, fx, c, progs=progs):
                R.check(c, got, model, "oracle", frac=1.0 / 8, keep=keep, limit=R.limit_more({"header": header}, model))
    # the variance-clip rule on the new cases
    pairs = removed = 0
    for c in fxm["kprog"]:
        keep = R.keep_mask(c)
        pairs += keep.size
        removed += int((~keep).sum())
        if R.bar_var(c) <= 1e-9:
            assert keep[0], f"{c['name']}: the candidate on a training point is removed at var bar {R.bar_var(c):.3g}"
    print(f"kprog candidates removed by the clip rule: {removed} of {pairs}")
    assert 4 * removed <= pairs, "more than a quarter of the kprog (case, candidate) pairs removed"
    header["kprog_clip_removed"] = [removed, pairs]

    flat, at, lines = [], 0, ['{"header":' + json.dumps(header, separators=(",", ":"))]
    for model in R.MODELS_MORE:
        rows = []
        for c in fxm[model]:
            layout = R.more_layout(model, fx["plain" if model == "kprog" else model]["datasets"][c["data"]])
            if model == "kprog":
                entry_ = {k: c[k] for k in ("data", "closure", "lam_rel", "amp", "sig", "mean", "cond")}
            else:
                entry_ = {"case": c["name"]}
            entry_["at"] = at
            for k, shp in layout:
                assert np.shape(c[k]) == shp, (k, np.shape(c[k]), shp)
                flat.append(np.asarray(c[k], dtype=np.float64).reshape(-1))
                at += flat[-1].size
            rows.append(json.dumps(entry_, separators=(",", ":")))
        lines.append(f',"{model}":[')
        lines += [ln + "," for ln in rows[:-1]] + [rows[-1] + "]"]
    with open(R.PATH_MORE, "w") as f:
        f.write("\n".join(lines) + "}\n")
    np.save(R.ARRAYS_MORE, np.concatenate(flat))
    sizes = os.path.getsize(R.PATH_MORE), os.path.getsize(R.ARRAYS_MORE)
    print("wrote", R.PATH_MORE, "and", R.ARRAYS_MORE, sizes, "bytes")
    assert max(sizes) < CAP, "each file of the fixture must stay below the project's cap"


if __name__ == "__main__":
    main()
