"""What the GPU tests of appended model handles (tests/test_gpu_appended_sets.py, tests/test_gpu_appended_large.py) rest on, checked
with the oracle alone (no GPU):

1 their references can tell right from wrong: the one bug those tests exist for — the appended points' rows read component-major,
  as if nhead == npts — moves μ, ∇μ and the set acquisition gradient by a large multiple of the bound the GPU test applies;
2 their condition-aware tolerances stay at or below those of the tests the bounds were taken from, so no bound is too loose to fail;
3 the Capacity rule predicts the append path, the growth and the block rows rebuilt that the GPU tests claim for every append;
4 the all-pairs forms of the oracle's cross-covariance and likelihood gradient (used where the pair loops take tens of seconds)
  agree with the pair loops.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import gp_oracle as O           # noqa: E402
import test_gpu_appended_large as TL        # noqa: E402
import test_gpu_appended_sets as TS         # noqa: E402
import test_gpu_ggp_append_track as GA      # noqa: E402
import test_gpu_ngp_append_track as NA      # noqa: E402
import test_gpu_ngp_grad_set as NG          # noqa: E402


def cond_tol(K, factor=8):
    return max(1e-9, np.linalg.cond(K) * K.shape[0] * 2.0 ** -53 * factor)


# ------------------------------------------------------------------------------------------ 1: sensitivity
def misread_tail(y, dY, nhead):
    """The observations of a handle whose appended points' rows are read component-major: the stored tail is point-major
    (y_j, ∂₁y_j, …, ∂_d y_j per appended point j); read as [y; ∂₁y; …; ∂_d y] of the nt appended points it hands out other numbers."""
    d, n = dY.shape
    nt = n - nhead
    stored = np.concatenate([np.concatenate([[y[nhead + j]], dY[:, nhead + j]]) for j in range(nt)])
    y2, dY2 = y.copy(), dY.copy()
    y2[nhead:] = stored[:nt]
    for l in range(d):
        dY2[l, nhead:] = stored[(1 + l) * nt:(2 + l) * nt]
    return y2, dY2


def test_the_references_tell_the_mixed_ordering_from_the_component_major_one():
    """Measured on the CPU (oracle alone), as multiples of the bound the GPU test applies to the same quantity:
      case 1(a), 65 points of which 5 appended, per sample s = 0, 1, 2:
        μ    (bound 1e-9)                              1.7e9, 1.4e9, 1.2e9   → asserted >= 1.2e8
        ∇μ   (bound 10 tol_s (1 + max|∇μ|))            1.2e7, 2.2e7, 4.5e7   → asserted >= 1.2e6
        set acquisition gradient, mode "both" (bound mean_s 100 tol_s (1 + max|∇acq_s|))   1.6e6   → asserted >= 1.6e5
      the large case with n0 reduced to 100 (appends [1, 8], 436 rows, λ = 0.45, (α, σ, σ_∂) = (1.2, 0.05, 0.1)):
        μ    (bound 1e-9)   2.0e9   → asserted >= 2.0e8;      ∇μ   (bound 10 tol (1 + max|∇μ|))   1.7e6   → asserted >= 1.7e5
    All margins are far above 100, so the data are rough enough.  The acquisition is not degenerate on these data: max acq 0.41,
    max|∇acq| 12.7 (asserted >= 0.1 and >= 1)."""
    D = TS.grad_data()
    n, nhead = TS.NT, TS.N0
    y_bad, dY_bad = misread_tail(D.Y[0, :n], D.dY[0][:, :n], nhead)
    assert np.abs(y_bad - D.Y[0, :n]).max() > 0.1
    bad_moments, margins_mu, margins_dmu = [], [], []
    for s in range(TS.S_):
        post, tol, mo = D.member(O, n, s, 0)
        lam, amp, sig, sgd = TS.hyper(s, 0)
        bad = O.gradient_gp_mean_and_var_grad(O.gradient_gp_fit(D.X[:, :n], y_bad, dY_bad, TS.KERNEL, lam, amp, sig, sgd), D.Xs)
        bad_moments.append(bad)
        margins_mu.append(np.abs(bad[0] - mo[0]).max() / 1e-9)
        margins_dmu.append(np.abs(bad[2] - mo[2]).max() / (10 * tol * (1 + np.abs(mo[2]).max())))
    y_max, best = TS.mode_args("both", 1, D.best)
    acq_o, dacq_o, ba, bg, _ = TS.oracle_set(O, D, [n] * TS.S_, 1, "both")
    res = [TS.compose(O, [m], [1.0], y_max, best) for m in bad_moments]
    dacq_bad = sum(r[1] for r in res) / len(res)
    margin_acq = np.abs(dacq_bad - dacq_o).max() / bg
    print(f"case 1(a): mu {['%.1e' % m for m in margins_mu]}  dmu {['%.1e' % m for m in margins_dmu]}  set acq grad {margin_acq:.1e}"
          f"  (max acq {acq_o.max():.2f}, max |dacq| {np.abs(dacq_o).max():.2f})")
    assert acq_o.max() >= 0.1 and np.abs(dacq_o).max() >= 1.0
    assert min(margins_mu) >= 1.2e8 and min(margins_dmu) >= 1.2e6 and margin_acq >= 1.6e5
    # the large gradient-observation case, n0 reduced from 300 to 100 (the oracle's candidate gradients loop over the pairs)
    n0, steps, more = TL.GGP_MAIN
    n0 = 100
    n = n0 + sum(steps)
    Dl = GA.Data(TL.D_, n)
    post = Dl.oracle(O, n, TL.LAM, TL.HYP)
    y_bad, dY_bad = misread_tail(Dl.y, Dl.dY, n0)
    bad = O.gradient_gp_mean_and_var_grad(O.gradient_gp_fit(Dl.X, y_bad, dY_bad, Dl.kernel, TL.LAM, *TL.HYP), Dl.Xs)
    good = O.gradient_gp_mean_and_var_grad(post, Dl.Xs)
    tol = cond_tol(O.augmented_kernel_matrix(Dl.kernel, Dl.X, TL.LAM, *TL.HYP))
    m_mu = np.abs(bad[0] - good[0]).max() / 1e-9
    m_dmu = np.abs(bad[2] - good[2]).max() / (10 * tol * (1 + np.abs(good[2]).max()))
    print(f"large case (n0 = 100): mu {m_mu:.1e}  dmu {m_dmu:.1e}")
    assert m_mu >= 2.0e8 and m_dmu >= 1.7e5


# ------------------------------------------------------------------------------------------ 2: the bounds can fail
def test_condition_aware_tolerances_stay_at_or_below_their_sources():
    """Per case of the GPU tests that uses tol = max(1e-9, cond(K) rows 2^-53 8): its largest tol against the largest tol of the test
    the bound was taken from, on that test's own data."""
    import test_gpu_acq_grad_set as GS
    D = TS.grad_data()
    mine = max([D.tol(O, TS.NT, s, p, other) for s in range(TS.S_) for p in range(2) for other in (False, True)] +
               [D.tol(O, TS.NT + 1, 0, p, True) for p in range(2)])     # (the member one point longer)
    src = 0.0
    for n, M in GS.GRAD_CASES:                                  # run_grad_model's members
        X, y, dY, lam, amp, sig, sgd = GS.grad_case(n, GS.D_, GS.S_, seed=n + M)
        src = max(src, max(cond_tol(O.augmented_kernel_matrix("matern52", X, lam[:, s], amp[s], sig[s], sgd[s])) for s in range(GS.S_)))
    print(f"gradient-observation sets: tol {mine:.2e} <= {src:.2e} (tests/test_gpu_acq_grad_set.py::run_grad_model)")
    assert mine <= src
    # the large gradient-observation case: ∇μ, ∇σ² after the re-update, against end_of_case over test_append_parity's cases
    n0, steps, more = TL.GGP_MAIN
    Dl = GA.Data(TL.D_, n0 + sum(steps) + more)
    mine = cond_tol(O.augmented_kernel_matrix(Dl.kernel, Dl.X, TL.LAM2, *TL.HYP2))
    src = 0.0
    for d, m0, st in GA.APPEND_CASES:
        Dd = GA.Data(d, m0 + sum(st))
        src = max(src, cond_tol(O.augmented_kernel_matrix(Dd.kernel, Dd.X, GA.lam_of(d), *GA.HYP)))
    print(f"gradient-observation handle of 1240 rows: tol {mine:.2e} <= {src:.2e} (tests/test_gpu_ggp_append_track.py::end_of_case)")
    assert mine <= src
    # the large nonstationary case after the re-update, against tests/test_gpu_parity.py::test_nonstationary_gp_candidate_gradients
    N0, steps, more = TL.NGP_MAIN
    N = N0 + sum(steps) + more
    D2 = TL.BigData(TL.D_, N, NA.M_CAND, True, False, c=1.15)
    post = D2.oracle(O, N)
    mine = cond_tol(post.L @ post.L.T)
    import test_gpu_parity as GP
    src = 0.0
    for d, Np, M in [(1, 20, 5), (3, 300, 70), (8, 1100, 40), (16, 150, 33)]:
        X, y, _ = GP.make(d, Np, M, seed=14)
        f_lam, _, f_amp, _, f_noise = NG.latents(d, 1.0, 1.0)   # (the latent models of that test)
        post = O.nonstationary_fit(X, y, NG.ev(f_lam, X).T, NG.ev(f_amp, X), NG.ev(f_noise, X), mean=0.3 * X[0])
        src = max(src, cond_tol(post.L @ post.L.T))
    print(f"nonstationary handle of {N} rows: tol {mine:.2e} <= {src:.2e} (tests/test_gpu_parity.py::test_nonstationary_gp_candidate_gradients)")
    assert mine <= src


class _Closed:
    def close(self):
        pass


class _NoDevice:
    """stands in for the api where tests/test_gpu_ngp_grad_set.py's Case fits its members: the oracle side is all that is read here"""

    @staticmethod
    def ngp_fit_batch(X, y, lam, amp, noi, mean=None, disc=None):
        S = lam.shape[2]
        return [_Closed() for _ in range(S)], np.zeros(S), np.zeros(S, dtype=np.int32)


@pytest.mark.parametrize("disc", [None, [False, True, False]])
def test_nonstationary_set_tolerances_stay_at_or_below_their_source(disc):
    """the appended nonstationary set (260 observations, S = 3, P = 2) against tests/test_gpu_ngp_grad_set.py's own 260-observation case"""
    mine = NG.Case(_NoDevice, O, TS.NS_N, TS.NS_M, S=TS.S_, P=2, discrete=disc, seed=5).tol.max()
    src = NG.Case(_NoDevice, O, 260, 70, discrete=disc).tol.max()
    print(f"nonstationary sets (discrete {disc is not None}): tol {mine:.2e} <= {src:.2e}")
    assert mine <= src


# ------------------------------------------------------------------------------------------ 3: the shapes
def blocks(cap, N0, n):
    """(path, grown, block rows of 128 rebuilt) of an append of n rows to N0 under the Capacity rule; `cap` is updated"""
    before = cap.cap
    path = cap.path(N0, n)
    grown = cap.cap > before
    nblk = cap.cap // 128
    rows = (nblk - 1 if grown else (N0 + n - 1) // 128) - N0 // 128 + 1
    return path, grown, rows


@pytest.mark.parametrize("rows_per_point,n0,steps,want", [
    (4, TS.N0, TS.STEPS, [(1, False, 1), (1, True, 3)]),                  # 1(a), 1(b): 240 -> 244 -> 260 rows, 256 grows to 512
    (4, TS.N0, [5], [(1, True, 3)]),                                      # 1(c): 60 + 5 points in one append
    (4, TS.N0, TS.STEPS + [1], [(1, False, 1), (1, True, 3), (1, False, 1)]),   # the unequal append: 260 -> 264 rows
    (1, TS.NS_N0, [10, 1], [(1, True, 3), (1, False, 1)]),                # nonstationary sets: 250 -> 260 -> 261
    (4, TL.GGP_MAIN[0], TL.GGP_MAIN[1] + [TL.GGP_MAIN[2]], [(1, False, 1), (1, False, 1), (1, False, 1)]),   # 1200 -> 1204 -> 1236 -> 1240 of 1280
    (4, TL.GGP_GROWTH[0], TL.GGP_GROWTH[1], [(1, True, 3)]),              # 1272 -> 1284: 1280 grows to 1536, three block rows
    (4, TL.GGP_PATH2[0], TL.GGP_PATH2[1], [(2, True, 6)]),                # 1040 -> 1600: six block rows, re-factorised
    (1, TL.NGP_MAIN[0], TL.NGP_MAIN[1] + [TL.NGP_MAIN[2]], [(1, False, 1), (1, False, 1), (1, False, 1)]),
    (1, TL.NGP_GROWTH[0], TL.NGP_GROWTH[1], [(1, True, 3)]),              # 1275 -> 1285
    (1, TL.NGP_PATH2[0], TL.NGP_PATH2[1], [(2, True, 6)]),                # 1030 -> 1630
])
def test_capacity_rule_predicts_the_claimed_paths(rows_per_point, n0, steps, want):
    assert GA.Capacity(1000).path(1000, 300) == NA.Capacity(1000).path(1000, 300)     # (the two copies of the rule agree)
    cap, N = GA.Capacity(n0 * rows_per_point), n0 * rows_per_point
    got = []
    for m in steps:
        got.append(blocks(cap, N, m * rows_per_point))
        N += m * rows_per_point
    assert got == want, got
    assert N <= 1630


def test_the_point_split_of_case_1a_straddles_nhead():
    """aug_grad_accum_set_kernel splits the points in min(…, (npts + 63) / 64) parts: 65 points give two, the second of which starts
    below nhead = 60 and ends above it, so one workgroup walks head rows (stride nhead) and appended rows (stride 1 + d)."""
    npts, nhead = TS.NT, TS.N0
    splits = (npts + 63) // 64
    assert splits == 2
    per = -(-npts // splits)
    lo, hi = per, npts - 1
    assert lo < nhead <= hi, (lo, hi)
    src = open(os.path.join(ROOT, "boss.jl_amd", "csrc", "host_predict.inc")).read()
    assert "nhead" in src and "predict_set_ok" in src


# ------------------------------------------------------------------------------------------ 4: the oracle's all-pairs forms
@pytest.mark.parametrize("kernel", ["matern32", "matern52", "sqexp"])
def test_all_pairs_forms_agree_with_the_pair_loops(kernel):
    """with a duplicated training point and a candidate on a training point (the entries the reference evaluates at x_j + 1e-8)"""
    d, n, M = 3, 14, 9
    X, y, dY = GA.make_grad(d, n, seed=8)
    X[:, 9] = X[:, 4]
    y, dY = GA.obs(X)
    Xs = np.random.default_rng(2).uniform(0, 1, (d, M))
    Xs[:, 3] = X[:, 6]
    lam, hyp = GA.lam_of(d), (1.1, 0.06, 0.09)
    a, b = O.augmented_cross_cov(kernel, X, lam, hyp[0], Xs), O.augmented_cross_cov_allpairs(kernel, X, lam, hyp[0], Xs)
    assert np.abs(a - b).max() <= 4 * 2.0 ** -52 * np.abs(a).max(), np.abs(a - b).max()
    ll, gr = O.gradient_gp_loglike_grad(X, y, dY, kernel, lam, *hyp)
    ll2, gr2 = O.gradient_gp_loglike_grad_allpairs(X, y, dY, kernel, lam, *hyp)
    assert ll == ll2
    assert np.abs(gr - gr2).max() <= 1e-12 * (1 + np.abs(gr).max()), (gr, gr2)
