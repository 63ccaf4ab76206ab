"""The regimes fixture (tests/golden/regimes.json, written by tests/golden/make_regimes.py) on the host: it is the grid its generator
declares, the fp64 oracle stays within 1/8 of every bar of the 50-digit truths, and the bars have teeth — the oracle with the +1e-8
lift left out, and with the lift applied twice (every parameter moved by ∓1e-8), falls outside the bar of at least one output in at
least one case of each model.  Bars, layout and the clip rule: tests/regimes_cases.py.  No 50-digit arithmetic runs here."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import regimes_cases as R  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

MODELS = ("plain", "grad", "gibbs")


@pytest.fixture(scope="module")
def fx():
    return R.load()


def test_fixture_is_the_declared_grid(fx):
    import make_regimes as G
    ds = G.datasets()
    for model in MODELS:
        for name, D in ds[model].items():
            for k, a in D.items():
                assert np.array_equal(fx[model]["datasets"][name][k], a), (model, name, k)
    declared = {}
    for model, c in G.grid():
        declared.setdefault(model, []).append(c)
    dropped = set(fx["header"]["gibbs_dropped"])
    assert len(declared["plain"]) == 135 + 15 and len(declared["grad"]) == 96 and len(declared["gibbs"]) == 72
    assert 10 * len(dropped) <= len(declared["gibbs"])
    for model in MODELS:
        want = [c for c in declared[model] if c["name"] not in dropped]
        got = fx[model]["cases"]
        assert [c["name"] for c in got] == [c["name"] for c in want]
        for a, b in zip(got, want):
            assert all(a[k] == v for k, v in b.items()), a["name"]
            # the bars' ingredient: cond(K) of the fp64 matrix (its own rounding error is cond·u relative, 4e-6 at the worst case)
            assert abs(R.cond_of(O, model, fx, a) / a["cond"] - 1) <= 1e-3, (a["name"], a["cond"])
    # the plain grid: both sizes, a third with a prior mean, one candidate on a training point and one outside the hull
    plain = fx["plain"]["cases"]
    assert sum(c["mean"] for c in plain) == len(plain) // 3
    for D in fx["plain"]["datasets"].values():
        assert (D["Xs"][:, 0] == D["X"][:, 7]).all() and (D["Xs"][:, 1] > D["X"].max(1)).any()
    assert os.path.getsize(R.PATH) + os.path.getsize(R.ARRAYS) < 400045      # below gp_golden.json


def test_clip_rule_caps(fx):
    pairs = removed = 0
    for model in MODELS:
        for c in fx[model]["cases"]:
            keep = R.keep_mask(c)
            pairs += keep.size
            removed += int((~keep).sum())
            if model != "grad" and R.bar_var(c) <= 1e-9:
                assert keep[0], c["name"]
    print(f"removed {removed} of {pairs}")
    assert 4 * removed <= pairs and [removed, pairs] == fx["header"]["clip_removed"]


@pytest.mark.parametrize("model", MODELS)
def test_oracle_within_an_eighth_of_every_bar(fx, model):
    worst = {}
    for c in fx[model]["cases"]:
        r = R.check(c, R.oracle_outputs(O, model, fx, c), model, "oracle", frac=1.0 / 8)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(model, "worst oracle err/(B·scale):", {k: f"{v:.3g}" for k, v in worst.items()}, "(bars: 8, gradients 100; asserted: an eighth)")
    assert set(fx["header"]["oracle_worst_ratio"][model]) == set(worst)          # the generator's own record of the same figures


@pytest.mark.parametrize("shift", [-1e-8, 1e-8])
@pytest.mark.parametrize("model", MODELS)
def test_a_lift_error_is_caught(fx, model, shift):
    """Every parameter moved by ∓1e-8 (the lift left out / applied twice; the Gibbs model takes its latent values as given, so
    there it is the values that move): at least one case of the model must miss at least one bar.  Only the well-conditioned
    cases can tell (the bars grow with cond(K)), so the search goes through them in order of B and stops at the first catch."""
    caught = None
    for c in sorted(fx[model]["cases"], key=R.unit)[:40]:
        try:
            r = R.ratios(c, R.oracle_outputs(O, model, fx, c, shift=shift), model)
        except O.PosDefException:
            continue
        out = {k: v for k, v in r.items() if v > R.LIMIT[k]}
        if out:
            caught = (c["name"], out)
            break
    print(model, shift, "caught by", caught)
    assert caught is not None, f"no {model} case separates a {shift:+g} error on every parameter from the truth: the grid is too tame"
