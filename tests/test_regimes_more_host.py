"""The second regimes fixture (tests/golden/regimes_more.json, written by tests/golden/make_regimes_more.py) on the host: it is the grid
its generator declares, the caps hold, the fp64 oracle stays within 1/8 of every bar of the 50-digit truths, the multipliers in the
header follow from the oracle's recorded ratios by the generator's rule, and the bars have teeth — with every parameter moved by
∓1e-8 the oracle misses EVERY new quantity in at least one of the 40 best-conditioned cases of its model, and the Gibbs gradients
without the latent Jacobians miss theirs in a case of contrast > 1.  Bars, layout and the clip rule: tests/regimes_cases.py.  No
50-digit arithmetic runs here."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import regimes_cases as R  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

NEW_KEYS = {"plain": ("cov",), "grad": ("dmu", "dvar", "cov"), "gibbs": ("dmu", "dvar", "cov"),
            "kprog": ("logpdf", "mu", "var", "dmu", "dvar", "llgrad")}


@pytest.fixture(scope="module")
def fx():
    return R.load()


@pytest.fixture(scope="module")
def fxm():
    return R.load_more()


@pytest.fixture(scope="module")
def progs():
    entry.build()
    import boss_jl_amd as B
    return R.kprog_programs(B)


def test_fixture_is_the_declared_grid(fx, fxm, progs):
    import make_regimes_more as G
    for model in ("plain", "grad", "gibbs"):                     # every case of the first fixture, in its order, by name
        assert [c["name"] for c in fxm[model]] == [c["name"] for c in fx[model]["cases"]]
    assert len(fxm["plain"]) == 150 and len(fxm["grad"]) == 96 and len(fxm["gibbs"]) == 72 - len(fx["header"]["gibbs_dropped"])
    declared = G.kprog_grid()
    assert len(declared) == 60 + 12
    assert sum(c["data"] == "a" for c in declared) == 60 and {c["closure"] for c in declared} == set(R.KPROG_CLOSURES)
    assert sum(c["mean"] for c in declared) == len(declared) // 3
    dropped = set(fxm["header"]["kprog_dropped"])
    assert 10 * len(dropped) <= len(declared)
    for c in declared:
        c.update(R.kprog_derived(fx["plain"]["datasets"][c["data"]], c))
    want = [c for c in declared if c["name"] not in dropped]
    assert [c["name"] for c in fxm["kprog"]] == [c["name"] for c in want]
    for a, b in zip(fxm["kprog"], want):
        assert all(a[k] == v for k, v in b.items()), a["name"]
        X, y, Xs, lam, amp, sig, mX, ms = R.plain_inputs(fx, a)
        cond = R.kprog_oracle(progs[(a["closure"], X.shape[0])], a, X, y, Xs, lam, amp, sig, mX, ms)[1]
        assert abs(cond / a["cond"] - 1) <= 1e-3, (a["name"], a["cond"])
        # expo leaves the candidate on a training point out of its gradients, and nothing else is left out anywhere
        for k in ("dmu", "dvar"):
            left_out = ~np.isfinite(a[k])
            assert left_out[:, list(R.no_grad_at(a))].all() and left_out.sum() == a[k].shape[0] * len(R.no_grad_at(a)), (a["name"], k)
        assert all(np.isfinite(a[k]).all() for k in ("logpdf", "mu", "var", "llgrad"))
    for model in ("plain", "grad", "gibbs"):
        assert all(np.isfinite(c[k]).all() for c in fxm[model] for k in NEW_KEYS[model])
    # the arrays file holds exactly what the layouts read, and both files stay below the project's cap
    n = sum(int(np.prod(shp)) for model in R.MODELS_MORE for c in fxm[model]
            for _, shp in R.more_layout(model, fx["plain" if model == "kprog" else model]["datasets"][c["data"]]))
    assert np.load(R.ARRAYS_MORE).shape == (n,)
    assert os.path.getsize(R.PATH_MORE) < 400000 and os.path.getsize(R.ARRAYS_MORE) < 400000


def test_clip_rule_caps(fxm):
    pairs = removed = 0
    for c in fxm["kprog"]:
        keep = R.keep_mask(c)
        pairs += keep.size
        removed += int((~keep).sum())
        if R.bar_var(c) <= 1e-9:
            assert keep[0], c["name"]
    print(f"removed {removed} of {pairs}")
    assert 4 * removed <= pairs and [removed, pairs] == fxm["header"]["kprog_clip_removed"]


@pytest.mark.parametrize("model", R.MODELS_MORE)
def test_oracle_within_an_eighth_of_every_bar(fx, fxm, progs, model):
    worst, limit = {}, R.limit_more(fxm, model)
    for c in fxm[model]:
        for got, keep in R.oracle_more(O, model, fx, c, progs=progs):
            for k, v in R.check(c, got, model, "oracle", frac=1.0 / 8, keep=keep, limit=limit).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(model, "worst oracle err/(B·scale):", {k: f"{v:.3g}" for k, v in worst.items()}, "multipliers:", {k: limit[k] for k in worst})
    recorded = fxm["header"]["oracle_worst_ratio"][model]
    assert set(recorded) == set(worst) == set(NEW_KEYS[model]) == set(fxm["header"]["multiplier"][model])
    for k in worst:                                              # the multipliers are the rule applied to the oracle's own record
        assert limit[k] == R.multiplier_of(k, recorded[k]), (k, limit[k], recorded[k])


@pytest.mark.parametrize("shift", [-1e-8, 1e-8])
@pytest.mark.parametrize("model", R.MODELS_MORE)
def test_a_lift_error_is_caught_in_every_new_quantity(fx, fxm, progs, model, shift):
    """Every parameter moved by ∓1e-8 (the lift left out / applied twice; Gibbs: the latent values move): each new quantity must miss
    its bar in at least one of the 40 best-conditioned cases of its model."""
    limit = R.limit_more(fxm, model)
    caught = {}
    for c in sorted(fxm[model], key=R.unit)[:40]:
        try:
            outs = R.oracle_more(O, model, fx, c, shift=shift, progs=progs)
        except (O.PosDefException, O.DomainError, np.linalg.LinAlgError):
            continue
        for got, keep in outs:
            for k, v in R.ratios(c, got, model, keep).items():
                if v > limit[k] and k not in caught:
                    caught[k] = (c["name"], float(f"{v:.3g}"))
        if set(caught) == set(NEW_KEYS[model]):
            break
    print(model, shift, "caught by", caught)
    missing = set(NEW_KEYS[model]) - set(caught)
    assert not missing, f"no {model} case separates a {shift:+g} error on every parameter from the truth of {sorted(missing)}: the grid is too tame"


def test_the_gibbs_chain_through_the_latent_jacobians_is_caught(fx, fxm):
    """dmu / dvar from the oracle called with dlam_Xs = damp_Xs = None (the ∂λ/∂x and ∂α/∂x terms dropped) miss the bar in at least one
    case of contrast > 1, for each of the two."""
    limit = R.limit_more(fxm, "gibbs")
    caught = {}
    for c in sorted(fxm["gibbs"], key=R.unit):
        if c["clam"] == 1 and c["camp"] == 1:
            continue
        for got, keep in R.oracle_more(O, "gibbs", fx, c, jacobians=False):
            for k in ("dmu", "dvar"):
                v = R.ratios(c, {k: got[k]}, "gibbs", keep)[k]
                if v > limit[k] and k not in caught:
                    caught[k] = (c["name"], float(f"{v:.3g}"))
        if len(caught) == 2:
            break
    print("caught by", caught)
    assert set(caught) == {"dmu", "dvar"}
