"""CPU tests of the acquisition-tail fixture (tests/golden/acq_tails.json, tests/acq_tails_cases.py): the fp64 oracle holds the bars at
its own recorded ratio, acquisition.feas_prob_host holds them on the feasibility groups, the truths regenerate, and six deliberately
wrong variants of the oracle each miss the bar somewhere — the bars have teeth where the absolute tolerances of the older tests
(1e-10 on values whose size is 1e-20 … 1e-300) have none.  The device is held to the same fixture by tests/test_gpu_acq_tails.py."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acq_tails_cases as A  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return A.load()


def results(g, mutant=None):
    """[(what, got, want, cond)] of the fp64 oracle (or a mutant) on a group."""
    if g["kind"] == "value":
        return [("value", A.oracle_value(O, g, mutant), g["truth"], g["cond"])]
    acq, dacq = A.oracle_grad(O, g, mutant)
    return [("value", acq, g["truth"], g["cond"]), ("grad", dacq, g["gtruth"], g["gcond"])]


def test_fixture_header_layout_and_size(fx):
    assert os.path.getsize(A.PATH) < A.SIZE_LIMIT
    h = fx["header"]
    assert h["u"] == A.U and h["dps"] == 50 and h["groups"] == len(fx["groups"])
    assert h["candidates"] == sum(g["M"] for g in fx["groups"])
    for k in ("value", "grad"):
        assert 1.0 <= h["oracle_ratio"][k] <= 4.0, "a first-order bar: the fp64 oracle sits within a few u·cond of the truth"
        assert h["device_C"][k] == A.device_C(h["oracle_ratio"][k]) and h["device_C"][k] >= 4 * h["oracle_ratio"][k]
        assert h["oracle_ratio_at"][k] in fx["by_name"]
    with open(A.PATH) as f:
        lines = f.read().splitlines()
    assert len(lines) == 1 + len(fx["groups"]) and lines[0].startswith('{"header":'), "one group per line behind the header"
    assert lines[-1].endswith("]}") and all(ln.endswith(",") for ln in lines[1:-1])
    for ln, g in zip(lines[1:-1] + [lines[-1][:-2]], fx["groups"]):
        o = json.loads(ln.rstrip(","))
        assert o["name"] == g["name"]
        assert ("twin" in o) == (g["twin"] is not None)
    names = set(fx["by_name"])
    assert {"ei-p2", "ei-p3", "ei-p16", "ei-p17", "ei-p20", "fp-1", "fp-2", "eifp", "eifp-tiny", "s3-tail", "s3-eifp", "g-tail-d1",
            "g-tail-d3", "g-ei-p16", "g-ei-p17", "g-ei-p20", "g-fp-1", "g-fp-2", "g-eifp"} <= names
    assert sum(n.startswith("tail-") for n in names) == 18
    for g in fx["groups"]:
        assert g["M"] <= 2100 and g["S"] in (1, 3) and g["d"] in ((1, 3) if g["kind"] == "grad" else (0,))
        if g["kind"] == "grad":
            assert g["var"].min() >= 1e-18 and (g["y_max"] is None or not np.isneginf(g["y_max"]).any())


def test_oracle_within_its_recorded_ratio(fx):
    h = fx["header"]["oracle_ratio"]
    seen = {"value": 0.0, "grad": 0.0}
    for g in fx["groups"]:
        if g["check"] == "tiny":
            assert A.check_tiny(A.oracle_value(O, g)), g["name"]
            continue
        for what, got, want, cond in results(g):
            bad = A.misses(got, want, cond, h[what] * (1 + 1e-9))          # (the recorded quotient, multiplied back: a rounding or two)
            assert not bad.any(), f"{g['name']} {what}: err/(u·cond) = {A.ratio(got, want, cond):.3g} > {h[what]:.3g} at {np.argwhere(bad)[:4].tolist()}"
            seen[what] = max(seen[what], A.ratio(got, want, cond))
    assert seen == h, "the recorded figures are the measured ones"


def test_feas_prob_host_on_the_feasibility_groups(fx):
    from boss_jl_amd import acquisition
    C = fx["header"]["oracle_ratio"]["value"]
    n = 0
    for g in fx["groups"]:
        if g["kind"] != "value" or g["best"] is not None or g["y_max"] is None:
            continue
        var = np.where((g["var"][0] < 0) & (g["var"][0] >= -1e-8), 0.0, g["var"][0])
        got = np.asarray(acquisition.feas_prob_host(g["mu"][0], var, g["y_max"]))
        assert not A.misses(got, g["truth"], g["cond"], C).any(), f"{g['name']}: err/(u·cond) = {A.ratio(got, g['truth'], g['cond']):.3g}"
        n += 1
    assert n >= 3


def test_truths_regenerate(fx):
    pytest.importorskip("mpmath")
    from oracle import mp_oracle as MP
    for g in fx["groups"]:
        if g["twin"]:
            continue
        for j in sorted(set(int(t) for t in np.linspace(0, g["M"] - 1, 5))):
            t = A.column_truth(MP, g, j)
            same = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)   # noqa: E731
            assert same(t[0], g["truth"][j]) and same(t[1], g["cond"][j]), (g["name"], j, t[:2], g["truth"][j], g["cond"][j])
            if g["kind"] == "grad":
                assert same(t[2], g["gtruth"][:, j]) and same(t[3], g["gcond"][:, j]), (g["name"], j)


# where each mutant must be caught: (group prefix, what)
TEETH = {"phi_erf": ("tail-", "value"), "pdf_f32": ("tail-", "value"), "unclipped": ("ei-p", "value"), "no_zero_branch": ("corners", "value"),
         "neginf_skipped": ("fp-neginf", "value"), "missing_half": ("g-", "grad")}


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_mutants_miss_the_bar(fx, mutant):
    """Each wrong variant misses the DEVICE's bar (4× the oracle's ratio, rounded up to a power of two) on at least one case of the
    group kind named in TEETH; printed: where, and by how much."""
    C = fx["header"]["device_C"]
    prefix, what_due = TEETH[mutant]
    caught = []
    for g in fx["groups"]:
        if g["check"] == "tiny" or (mutant == "missing_half" and g["kind"] != "grad"):
            continue
        for what, got, want, cond in results(g, mutant):
            bad = A.misses(got, want, cond, C[what])
            if bad.any():
                caught.append((g["name"], what, int(bad.sum()), A.ratio(got, want, cond)))
    print(f"{mutant}: " + "; ".join(f"{n} {w}: {k} candidates, worst err/(u·cond) {r:.3g}" for n, w, k, r in caught))
    assert any(n.startswith(prefix) and w == what_due for n, w, _, _ in caught), f"{mutant} passes every bar of the {prefix}* groups"
    if mutant == "phi_erf":
        # the issue's point: it passes the older absolute tolerance on every tail case
        for g in fx["groups"]:
            if g["name"].startswith("tail-"):
                assert np.allclose(A.oracle_value(O, g, mutant), g["truth"], rtol=0, atol=1e-10 * max(1.0, float(np.sqrt(g["var"].max()))))
    # the unmutated oracle is back
    g = fx["by_name"]["tail-s1-b0"]
    assert not A.misses(A.oracle_value(O, g), g["truth"], g["cond"], fx["header"]["oracle_ratio"]["value"]).any()
