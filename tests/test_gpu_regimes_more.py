"""GPU tests (pytest -m gpu) of further device outputs over the hyper-parameter range, against 50-digit truths: posterior covariances of
the three models, candidate gradients of the gradient-observation model (GP.predict_grad on a GradGP handle) and of the Gibbs model
(with the chain through the latent Jacobians), and program-kernel posteriors (KernelGP: update, predict, loglike_grad, predict_grad).

Inputs come only from tests/golden/regimes.json and tests/golden/regimes_more.json (generated on the CPU by make_regimes.py and
make_regimes_more.py; no 50-digit arithmetic runs here) through tests/regimes_cases.py.  With B = cond(K)·rows·u, u = 2⁻⁵³:

    cov entries  m·B·amp2     every gradient  m·B·(1 + max|want|)     kprog logpdf, μ, var  as the plain model's

m = 8 and 100, or the larger power of two the fixture's header records where the fp64 oracle itself does not stay within an eighth of
that (chosen from the oracle alone; regimes_cases.limit_more).  Every test prints err/(B·scale) per case and quantity.  Candidates
whose true variance is within 2 bars + 1e-8 of zero are left out of the calls that clip (regimes_cases.keep_mask); predict_value_cov,
which does not clip, gets every candidate.  A BOSS_E_NOT_PD or BOSS_E_NEG_VAR fails the test.

Shapes: those of tests/test_gpu_regimes.py — (d, N, M) = (2, 40, 6) and (3, 136, 9) for the plain and the program-kernel model, n = 12
and 45 points (36 and 135 rows) for the gradient model, N = 40 and 136 for the Gibbs model."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import regimes_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [("plain", "a"), ("plain", "b"), ("grad", "n12"), ("grad", "n45"), ("gibbs", "n40"), ("gibbs", "n136"), ("kprog", "a"), ("kprog", "b")]
NEW_KEYS = {"plain": ("cov",), "grad": ("dmu", "dvar", "cov"), "gibbs": ("dmu", "dvar", "cov"),
            "kprog": ("logpdf", "mu", "var", "dmu", "dvar", "llgrad")}


@pytest.fixture(scope="module")
def B():
    import __graft_entry__ as entry
    entry.build()
    import boss_jl_amd as B
    B.api.load_library()
    assert B.api.device_count() >= 1
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def fx():
    return R.load()


@pytest.fixture(scope="module")
def fxm():
    return R.load_more()


@pytest.fixture(scope="module")
def progs(B):
    return R.kprog_programs(B)


def new_handle(api, fx, progs, model, c):
    D = fx["plain" if model == "kprog" else model]["datasets"][c["data"]]
    if model == "plain":
        return api.GP(D["X"], D["y"], c["kernel"])
    if model == "grad":
        return api.GradGP(D["X"], D["y"], D["dY"], c["kernel"])
    if model == "gibbs":
        return api.GibbsGP(D["X"], D["y"])
    return api.KernelGP(D["X"], D["y"], progs[(c["closure"], D["X"].shape[0])], grad=True)


def fmt(r):
    return " ".join(f"{k} {v:.3g}" for k, v in r.items())


@pytest.mark.parametrize("model,data", SIZES)
def test_handles_against_the_further_truths(api, fx, fxm, progs, model, data):
    """predict_cov (plain: Σ and its diagonal, bitwise symmetric), GP.predict_grad on a GradGP handle and predict_value_cov,
    GibbsGP.predict_grad with the closed-form Jacobians (without them where they vanish) and predict_cov, KernelGP(grad=True) update /
    predict / loglike_grad / predict_grad: every regime of the grid, one resident handle per kernel or closure re-fitted from regime
    to regime as a fitter does."""
    handles, failures, limit = {}, [], R.limit_more(fxm, model)
    try:
        for c in [c for c in fxm[model] if c["data"] == data]:
            key = c.get("kernel", c.get("closure"))
            if key not in handles:
                handles[key] = new_handle(api, fx, progs, model, c)
            for what, got, keep in R.DEVICE_MORE[model](api, fx, c, handles[key], progs=progs):
                kept = "all" if keep is None else f"{int(keep.sum())}/{keep.size}"
                print(f"{c['name']} cond {c['cond']:.3g} kept {kept} {what}: {fmt(R.ratios(c, got, model, keep))}")
                try:
                    R.check(c, got, model, what, keep=keep, limit=limit)
                except AssertionError as e:
                    failures.append(str(e))
    finally:
        for h in handles.values():
            h.close()
    assert not failures, f"{len(failures)} misses:\n" + "\n".join(failures[:40])


@pytest.mark.parametrize("data", ["a", "b"])
@pytest.mark.parametrize("closure", R.KPROG_CLOSURES)
def test_kprog_batches_equal_the_handles_bitwise(api, fx, fxm, progs, closure, data):
    """kgp_loglike_batch over all regimes of a closure as one batch of S sets (a third of them with their prior mean, the others with a
    zero row): the bits of KernelGP.update at the same parameters, hence within the truth bars by the test above."""
    cs = [c for c in fxm["kprog"] if c["data"] == data and c["closure"] == closure]
    inp = [R.plain_inputs(fx, c) for c in cs]
    X, y = inp[0][0], inp[0][1]
    lam = np.asfortranarray(np.stack([i[3] for i in inp], axis=1))
    amp, sig = np.array([i[4] for i in inp]), np.array([i[5] for i in inp])
    means = np.stack([np.zeros(X.shape[1]) if i[6] is None else i[6] for i in inp])
    prog = progs[(closure, X.shape[0])]
    h = api.KernelGP(X, y, prog, grad=True)
    try:
        lp_h = np.array([h.update(i[3], i[4], i[5], i[6]) for i in inp])
    finally:
        h.close()
    ll, st = api.kgp_loglike_batch(X, y, prog, lam, amp, sig, mean_X=means)
    print(f"{data} {closure}: S = {len(cs)}, max |ll − handle| {np.abs(ll - lp_h).max():.3g}")
    assert not st.any(), st
    assert np.array_equal(ll, lp_h)


@pytest.mark.parametrize("shift", [-1e-8, 1e-8])
@pytest.mark.parametrize("model", R.MODELS_MORE)
def test_a_lift_error_on_the_device_would_be_caught(api, fx, fxm, progs, model, shift):
    """The comparison above has teeth on the device's own results: handed parameters that are off by ∓1e-8 (what a +1e-8 lift left out
    or applied twice on one path amounts to), the device misses the bar of a NEW quantity in at least one of the 10 best-conditioned
    cases of each group."""
    limit = R.limit_more(fxm, model)
    caught = None
    for c in sorted(fxm[model], key=R.unit)[:10]:
        for what, got, keep in R.DEVICE_MORE[model](api, fx, c, None, shift, progs=progs):
            out = {k: v for k, v in R.ratios(c, got, model, keep).items() if k in NEW_KEYS[model] and v > limit[k]}
            if out and caught is None:
                caught = (c["name"], what, out)
    print(model, shift, "caught by", caught)
    assert caught is not None
