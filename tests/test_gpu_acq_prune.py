"""The arg-max-only acquisition path (csrc/host_prune.inc, csrc/prune_kernels.hpp), pytest -m gpu.

boss_acq_ei without acq_out bounds every candidate's EI from above (exact mean, variance after the first s row blocks), finishes
the K largest bounds exactly, and then only what their maximum cannot exclude.  Every test makes the pruned call and a
want_acq = True call (the full kernel) on the same handle and asks for the same arg-max and
|max − acq[argmax]| <= 1e-12 (1 + |max|), the tolerance of tests/test_gpu_parity.py for the few-candidates path against the
fused kernel.  The thresholds are lowered through boss_debug_acq_prune_set so that small shapes reach the path.
(The reference's sampling maximizer evaluates all candidates and takes argmax: src/acquisition_maximizers/sampling.jl:43-57.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL, PRUNED, FALLBACK, SKIPPED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(autouse=True)
def small_thresholds(api):
    api._acq_prune_set(0, min_tiles=0, K=64, s=2, cap=1024, slack=1.0)
    yield
    api._acq_prune_set(0, min_tiles=-2, K=-2, s=-2, cap=-2, slack=1.0)


def problem(N, d, M, seed):
    """the problems of tests/test_acq_prune_bound.py"""
    rng = np.random.default_rng(100 + seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = np.random.default_rng(200 + seed).uniform(0, 1, (d, M))
    return X, y, Xs


_handles = {}


def fitted(api, N, d, M, seed, kernel="matern52", noise=0.05, mean=False):
    """one fitted handle and candidate set per problem, shared by the tests that leave it unchanged"""
    key = (N, d, M, seed, kernel, noise, mean)
    if key not in _handles:
        X, y, Xs = problem(N, d, M, seed)
        g = api.GP(X, y, kernel)
        g.update(np.full(d, 0.5), 1.0, noise, mean_X=0.3 * X[0] if mean else None)
        _handles[key] = (g, api.Candidates(Xs), X, y, Xs)
    return _handles[key]


def both(api, g, cand, coef, best, mask=None, mean_Xs=None):
    """(pruned call's (argmax, max), its path report, the full call's acq)"""
    _, am, mx = api.acq_ei([[g]], cand, [coef], None, best, valid_mask=mask, mean_Xs=mean_Xs, want_acq=False)
    rep = api._acq_path(0)
    acq, am_f, mx_f = api.acq_ei([[g]], cand, [coef], None, best, valid_mask=mask, mean_Xs=mean_Xs, want_acq=True)
    print(f"path {rep}  pruned ({am}, {mx!r})  full ({am_f}, {mx_f!r})  |max - acq[argmax]| {abs(mx - acq[am_f]):.3e}")
    return (am, mx), rep, (acq, am_f, mx_f)


def same(pruned, full):
    (am, mx), (acq, am_f, mx_f) = pruned, full
    assert am == am_f, (am, am_f, mx, mx_f)
    if np.isnan(mx_f):
        assert np.isnan(mx)
    else:
        assert abs(mx - acq[am_f]) <= 1e-12 * (1 + abs(mx)), (mx, acq[am_f])


def bound_holds(api, M, full):
    """With the slacks in place no candidate's bound lies below its exact value (a NaN bound passes: its candidate always survives).
    Below the smallest normal number the EI formula's products round in denormals, so a bound may sit an ulp or two of 5e-324 under
    the exact value there (the survivor rule allows for it): the comparison gives that range away, nothing more."""
    mua, vs, ub = api._acq_prune_bounds(M)
    acq = full[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        short = ub < acq - np.finfo(float).tiny
        print(f"min(ub - acq) {float(np.nanmin(ub - acq)):.3e}  min(ub/acq) {float(np.nanmin(np.where(acq > 0, ub / acq, np.inf))):.6f}")
    assert not short.any(), (np.flatnonzero(short)[:8], ub[short][:8], acq[short][:8])


# ------------------------------------------------------------------------------------------ 1: kernels and options
@pytest.mark.parametrize("kernel,N,d,M,coef,mean,masked", [
    ("matern32", 1024, 3, 2100, 1.0, False, False),
    ("matern52", 1100, 3, 4131, 1.0, False, True),          # N no multiple of 256 (padded to 1280), M no multiple of 32, a domain mask
    ("sqexp", 1536, 8, 2100, 1.0, False, False),
    ("matern52", 1024, 8, 2100, -1.0, False, False),        # negative fitness coefficient
    ("matern32", 1100, 8, 300, 1.0, True, False),           # prior means at the points and at the candidates
    ("matern52", 1536, 3, 4131, -1.0, True, True),
])
def test_kernels_and_options(api, kernel, N, d, M, coef, mean, masked):
    g, cand, X, y, Xs = fitted(api, N, d, M, 0, kernel, mean=mean)
    best = float((coef * y).max())
    mask = None
    if masked:
        mask = np.random.default_rng(5).uniform(size=M) > 0.3
    mean_Xs = (0.3 * Xs[0])[None, None, :] if mean else None
    pruned, rep, full = both(api, g, cand, coef, best, mask, mean_Xs)
    same(pruned, full)
    assert rep[0] == PRUNED and rep[1] == 64 and rep[3] == 2, rep
    bound_holds(api, M, full)


@pytest.mark.parametrize("N,d,M", [(1100, 3, 4200), (1536, 6, 2100), (1024, 8, 8192)])
def test_few_contenders_at_the_incumbent(api, N, d, M):
    """best = y.max(), s = 2: the numpy restatement finishes 64 + 0 candidates on these problems; M/8 leaves the device room"""
    g, cand, X, y, Xs = fitted(api, N, d, M, 0)
    pruned, rep, full = both(api, g, cand, 1.0, float(y.max()))
    same(pruned, full)
    assert rep[0] == PRUNED and rep[1] + rep[2] <= M // 8, rep
    bound_holds(api, M, full)


# ------------------------------------------------------------------------------------------ 2: exploration regime
def test_round_two_fallback_and_back_off(api):
    g, cand, X, y, Xs = fitted(api, 1100, 3, 4200, 3)
    best = float(y.max()) + 1.0
    api._acq_prune_set(0, s=1)                             # (the numpy restatement leaves 431 contenders behind round 1 here)
    pruned, rep, full = both(api, g, cand, 1.0, best)
    same(pruned, full)
    assert rep[0] == PRUNED and rep[2] > 0 and rep[3] == 1, rep
    bound_holds(api, 4200, full)
    # cap = 0: every attempt falls back, with identical results, and pauses 1, 2, 4 … calls
    api._acq_prune_set(0, cap=0)
    paths = []
    for _ in range(10):
        _, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
        paths.append(api._acq_path(0)[0])
        assert am == full[1] and mx == full[2]             # (the full kernel's own result: bit for bit)
    assert paths == [FALLBACK, SKIPPED, FALLBACK, SKIPPED, SKIPPED, FALLBACK, SKIPPED, SKIPPED, SKIPPED, SKIPPED], paths
    # the first success resets the pause
    api._acq_prune_set(0, cap=1024)
    _, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
    assert api._acq_path(0)[0] == PRUNED and am == full[1]
    api._acq_prune_set(0, cap=0)
    paths = []
    for _ in range(3):
        api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
        paths.append(api._acq_path(0)[0])
    assert paths == [FALLBACK, SKIPPED, FALLBACK], paths
    api._acq_prune_set(0, cap=1024)
    for _ in range(3):                                     # (leave the shared handle without a pause)
        api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
    assert api._acq_path(0)[0] == PRUNED


# ------------------------------------------------------------------------------------------ 3: ties and edge cases
def test_ties_and_edge_cases(api):
    N, d, M = 1024, 3, 2100
    g, cand, X, y, Xs = fitted(api, N, d, M, 1)
    best = float(y.max())
    acq, am0, _ = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=True)
    assert 5 < am0 < M - 5
    # the winner once more at a lower and at a higher index: the first index wins
    Xd = Xs.copy()
    Xd[:, 3] = Xs[:, am0]
    Xd[:, M - 2] = Xs[:, am0]
    cd = api.Candidates(Xd)
    pruned, rep, full = both(api, g, cd, 1.0, best)
    same(pruned, full)
    assert pruned[0] == 3 and rep[0] == PRUNED
    # a NaN coordinate: the first NaN index wins (the cap is raised so that round 2 takes everything a NaN threshold leaves)
    Xn = Xs.copy()
    Xn[1, 777] = np.nan
    Xn[0, 1500] = np.nan
    cn = api.Candidates(Xn)
    api._acq_prune_set(0, cap=4096)
    pruned, rep, full = both(api, g, cn, 1.0, best)
    api._acq_prune_set(0, cap=1024)
    same(pruned, full)
    assert pruned[0] == 777 and np.isnan(pruned[1]) and rep[0] == PRUNED, (pruned, rep)
    # M copies of one point: index 0, by whichever path runs
    cc = api.Candidates(np.repeat(Xs[:, am0:am0 + 1], 300, axis=1))
    pruned, rep, full = both(api, g, cc, 1.0, best)
    same(pruned, full)
    assert pruned[0] == 0
    # all candidates masked: value 0, index 0
    pruned, rep, full = both(api, g, cand, 1.0, best, mask=np.zeros(M, dtype=bool))
    same(pruned, full)
    assert pruned == (0, 0.0)
    for _ in range(70):                                    # (whatever pause the fallbacks above left on the shared handle runs out)
        api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
        if api._acq_path(0)[0] == PRUNED:
            break
    assert api._acq_path(0)[0] == PRUNED


# ------------------------------------------------------------------------------------------ 4: staleness
def test_a_is_rebuilt_when_the_factor_changes(api):
    N, d, M = 1100, 3, 2100
    X, y, Xs = problem(N, d, M, 2)
    g = api.GP(X, y, "matern52")
    cand = api.Candidates(Xs)
    best = float(y.max())
    g.update(np.full(d, 0.5), 1.0, 0.05)
    pruned, rep, full = both(api, g, cand, 1.0, best)
    same(pruned, full)
    assert rep[0] == PRUNED and rep[4] == 1, rep
    first = pruned
    # the same factorisation again: a is reused, nothing is allocated, the few-candidates counter does not move, same bits
    api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
    c0 = api._acq_counters(g)
    for _ in range(3):
        _, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
        rep = api._acq_path(0)
        assert rep[0] == PRUNED and rep[4] == 0, rep
        assert (am, mx) == first
    c1 = api._acq_counters(g)
    assert c1[0] == 0 and c1[1] == c0[1] and c1[2] == c0[2], (c0, c1)
    assert c1[3] - c0[3] == 3 * 7 + 2 * 3 * (1 if rep[2] > 0 else 0), (c0, c1, rep)
    # another noise level, then an appended observation: a is stale each time
    g.update(np.full(d, 0.5), 1.0, 0.08)
    pruned, rep, full = both(api, g, cand, 1.0, best)
    same(pruned, full)
    assert rep[0] == PRUNED and rep[4] == 1, rep
    g.append(np.random.default_rng(9).uniform(0, 1, d), 0.1)
    pruned, rep, full = both(api, g, cand, 1.0, best)
    same(pruned, full)
    assert rep[0] == PRUNED and rep[4] == 1, rep


# ------------------------------------------------------------------------------------------ 5: switches
CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import __graft_entry__ as entry
entry.build()
from boss_jl_amd import api
import test_gpu_acq_prune as T
api._acq_prune_set(0, min_tiles=0)
g, cand, X, y, Xs = T.fitted(api, 1024, 3, 2100, 0)
pruned, rep, full = T.both(api, g, cand, 1.0, float(y.max()))
T.same(pruned, full)
assert rep[0] == 0, rep
print("RES ok")
"""


def test_switches(api):
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BOSS_ACQ_PRUNE="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RES ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    # an active profiling scope keeps the full kernel (bench.py --full times predict_kernel through the "predict" scope)
    g, cand, X, y, Xs = fitted(api, 1024, 3, 2100, 0)
    api.prof_enable(0, True)
    try:
        pruned, rep, full = both(api, g, cand, 1.0, float(y.max()))
    finally:
        api.prof_enable(0, False)
        api.prof_reset(0)
    same(pruned, full)
    assert rep[0] == FULL, rep


# ------------------------------------------------------------------------------------------ 6: slack self-check
def test_without_slack_in_an_ill_conditioned_regime(api):
    """noise 1e-6, slacks 0: the answer is still the full kernel's.  The run-time check compares μ_a with the mean of every finished
    candidate and fires where they differ by more than a tenth of the mean slack; a tenth of a zero slack is zero, so it fires where
    they differ at all, the attempt is discarded and the full kernel answers (path 2).  Only if every finished mean equals μ_a to the
    bit does the pruned result stand (path 1), and then the unslackened bound must have held where it decided: at the arg-max."""
    N, d, M = 1024, 3, 4131                                # (130 tiles: the full call is the fused kernel, the same bits every time)
    g, cand, X, y, Xs = fitted(api, N, d, M, 0, noise=1e-6)
    api._acq_prune_set(0, cap=4096, slack=0.0)             # (cap >= M: nothing but the mean check can discard the attempt)
    pruned, rep, full = both(api, g, cand, 1.0, float(y.max()))
    same(pruned, full)
    assert rep[0] in (PRUNED, FALLBACK), rep
    mua, vs, ub = api._acq_prune_bounds(M)
    mu, var = g.predict(Xs)
    dmu = float(np.max(np.abs(mua - mu)))
    print(f"path {rep}: max|mu_a - mu| {dmu:.3e}, min(ub - acq) {float(np.min(ub - full[0])):.3e}")
    if rep[0] == FALLBACK:
        assert dmu > 0.0                                   # (the mean check fired: the means do differ)
        assert pruned[1] == full[2]                        # (and the full kernel's own maximum came back, bit for bit)
    else:
        assert ub[full[1]] >= full[0][full[1]] * (1 - 1e-9)
    api._acq_prune_set(0, cap=1024, slack=1.0)
    for _ in range(3):                                     # (leave the shared handle without a pause)
        api.acq_ei([[g]], cand, [1.0], None, float(y.max()), want_acq=False)
    assert api._acq_path(0)[0] == PRUNED


def test_the_mean_check_fires_and_the_handle_backs_off(api):
    """The whole chain behind the run-time check: mean check, path 2, the full kernel's result, the pauses, the reset.
    μ_a = m + k*ᵀ(L⁻ᵀz) and the substitution's μ = (L⁻¹k*)ᵀz sum 1024 products in different orders, and at noise 1e-6 each carries
    a rounding error of about the condition number times 2⁻⁵³ relative: 64 finished means that all equal μ_a to the last bit do not
    happen, so with a zero slack the check fires on every attempt.
    The reset is shown after an update to noise 0.05 (the pause belongs to the handle and outlives the update): there the pruned
    call is held to the 1e-12 of every other test.  At noise 1e-6 itself the few-candidates path, which finishes the contenders,
    and the fused kernel differ by more than that (measured on the MI355X: same index, maxima 5.7e-12 apart at 2.77e-3), as they do
    for any call there; the index is asserted, the difference printed."""
    N, d, M = 1024, 3, 4131                                # (130 tiles: the full call is the fused kernel, the same bits every time)
    X, y, Xs = problem(N, d, M, 0)
    g = api.GP(X, y, "matern52")                           # (its own handle: the test changes its factorisation)
    g.update(np.full(d, 0.5), 1.0, 1e-6)
    cand = api.Candidates(Xs)
    best = float(y.max())
    api._acq_prune_set(0, cap=4096, slack=0.0)             # (cap >= M: nothing but the mean check can discard an attempt)
    pruned, rep, full = both(api, g, cand, 1.0, best)
    assert rep[0] == FALLBACK and rep[1] == 64 and rep[2] <= M - 64, rep
    assert pruned == (full[1], full[2])                    # (the full kernel's own result: bit for bit)
    paths = []
    for _ in range(6):
        _, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
        paths.append(api._acq_path(0)[0])
        assert (am, mx) == (full[1], full[2])
    assert paths == [SKIPPED, FALLBACK, SKIPPED, SKIPPED, FALLBACK, SKIPPED], paths
    # the slacks back: the attempt at this noise level would now stand
    api._acq_prune_set(0, cap=1024, slack=1.0)
    # another factorisation, the pause (4 calls, one of them spent) runs out, the attempt succeeds and the pause is reset
    g.update(np.full(d, 0.5), 1.0, 0.05)
    full = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=True)
    paths = []
    for _ in range(5):
        _, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=False)
        paths.append(api._acq_path(0)[0])
        same((am, mx), full)
    assert paths == [SKIPPED, SKIPPED, SKIPPED, PRUNED, PRUNED], paths
    # back at noise 1e-6 with the slacks in place the check stays quiet and the pruned call finds the full call's index
    g.update(np.full(d, 0.5), 1.0, 1e-6)
    pruned, rep, full = both(api, g, cand, 1.0, best)
    assert rep[0] == PRUNED and pruned[0] == full[1], (rep, pruned, full[1:])
    bound_holds(api, M, full)
