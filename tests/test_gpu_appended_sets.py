"""Set-wide calls over APPENDED model handles (pytest -m gpu): members of a gradient-observation or nonstationary set that have each
been appended the same points own their storage, have equal N, Np, ld, npts, ldx and nhead again, and so take the one-launch paths
(predict_set_enqueue, aug_grad_accum_set_kernel / gibbs_grad_accum_set_kernel) — for the gradient-observation model over the mixed
row ordering (the points given at creation component-major, every appended point's 1 + d rows in a run at the end).

The reference everywhere is the oracle on a fresh fit of ALL points in the reference's own row order [y; ∂₁y; …; ∂_d y].

Tolerances, each taken from the test that holds the same quantity to it on fresh handles:
  acq_ei against the oracle's sample mean          1e-10            tests/test_gpu_model_fit_batch.py:222
  acq_ei_grad_set, gradient-observation members    tol_s = max(1e-9, cond(K_s) rows 2^-53 8); |Δacq| <= 10 tol_s,
                                                   |Δ∇acq| <= 100 tol_s (1 + max|∇acq_s|), mean over s
                                                   tests/test_gpu_acq_grad_set.py:158-169 (run_grad_model); a sample of P outputs
                                                   takes the sum of its members' tol (tests/test_gpu_ngp_grad_set.py:10)
  set against the loop of acq_ei_grad              twice those bounds   tests/test_gpu_acq_grad_set.py:192-205
  predict / predict_grad of one handle             1e-9 on μ, σ²; 10 tol relative on ∇μ, ∇σ²   tests/test_gpu_ggp_append_track.py:92,135
  nonstationary members                            tests/test_gpu_ngp_grad_set.py:8-11,178-197 (assert_members, assert_acq, reused)
  _lat calls against their array twins             bit for bit          tests/test_gpu_nlat.py:288-310 (check_set_calls, reused)
tests/test_appended_sets_host.py shows on the CPU that these bounds tell the mixed ordering from the component-major one by a wide
margin, that the condition-aware tol of the data used here stays at or below that of the source tests, and that the Capacity rule
predicts the append paths claimed below.
"""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_ggp_append_track as GA      # noqa: E402  (Capacity, obs, make_grad, lam_of)
import test_gpu_ngp_grad_set as NG          # noqa: E402  (Case, assert_members, assert_acq, check_case)

pytestmark = pytest.mark.gpu
MODES = ("both", "best_only", "cons_only", "none")
KERNEL = "matern52"


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


@pytest.fixture(scope="module")
def B(api):
    import boss_jl_amd
    return boss_jl_amd


# ------------------------------------------------------------------------------------------ gradient-observation sets: the data
D_, S_, N0, STEPS, M_ = 3, 3, 60, [1, 4], 70
NT = N0 + sum(STEPS)                                            # 65 points, 260 rows; point 65 is the unequal append
Y_MAX = [0.5, 0.45]


def second_output(X):
    """the feasibility output of tests/test_gpu_ggp_append_track.py::test_sequential_batch_equals_the_oracle_loop"""
    y = 0.5 * np.cos(2 * X[0]) + 0.1 * np.sin(5 * X[1])
    dY = np.stack([-np.sin(2 * X[0]), 0.5 * np.cos(5 * X[1]), np.zeros(X.shape[1])])
    return y, dY


def hyper(s, p, other=False):
    """(λ, α, σ, σ_∂) of sample s, output p: λ and α of test_set_member_leaves_its_set, its noise levels doubled (so that the
    condition-aware tol stays below that of run_grad_model's own data, tests/test_appended_sets_host.py); `other`: the re-update"""
    c = (1.0, 1.1, 1.2)[s] * (1.0 + 0.05 * p) * (1.15 if other else 1.0)
    k = 0.9 if other else 1.0
    return GA.lam_of(D_, c), k * (1.1, 1.0, 0.9)[s], (0.06, 0.08, 0.10)[s] / k, (0.14, 0.16, 0.18)[s] / k


class GradSetData:
    """66 points of d = 3 with values and gradients of two outputs and 70 candidates: candidate 3 lies on head point 2, candidate 5 on
    appended point 62.  Oracle results are computed once per (points, output, sample, hyper-parameters) and kept."""

    def __init__(self):
        self.X = GA.make_grad(D_, NT + 1, seed=41)[0]
        y0, dY0 = GA.obs(self.X)
        y1, dY1 = second_output(self.X)
        self.Y, self.dY = np.stack([y0, y1]), np.stack([dY0, dY1])
        self.Xs = np.asfortranarray(np.random.default_rng(1041).uniform(0.05, 0.95, (D_, M_)))
        self.Xs[:, 3] = self.X[:, 2]
        self.Xs[:, 5] = self.X[:, 62]
        self.best = float(np.median(y0[:NT]))                   # (as tools/fuzz.py: EI is of order 0.1 at many candidates)
        self._memo = {}

    def member(self, O, n, s, p, other=False):
        """(post, tol, (μ, σ², ∇μ, ∇σ²) at the candidates) of the oracle's fit of the first n points"""
        key = (n, s, p, other)
        if key not in self._memo:
            lam, amp, sig, sgd = hyper(s, p, other)
            post = O.gradient_gp_fit(self.X[:, :n], self.Y[p, :n], self.dY[p][:, :n], KERNEL, lam, amp, sig, sgd)
            self._memo[key] = (post, self.tol(O, n, s, p, other), O.gradient_gp_mean_and_var_grad(post, self.Xs))
        return self._memo[key]

    def tol(self, O, n, s, p, other=False):
        """max(1e-9, cond(K) rows 2^-53 8) of that member (tests/test_gpu_acq_grad_set.py:158-159)"""
        K = O.augmented_kernel_matrix(KERNEL, self.X[:, :n], *hyper(s, p, other))
        return max(1e-9, np.linalg.cond(K) * K.shape[0] * 2.0 ** -53 * 8)


_GRAD_DATA = None


def grad_data():
    global _GRAD_DATA
    if _GRAD_DATA is None:
        _GRAD_DATA = GradSetData()
    return _GRAD_DATA


def mode_args(mode, P, best):
    return (Y_MAX[:P] if mode in ("both", "cons_only") else None), (best if mode in ("both", "best_only") else None)


def compose(O, moments, coefs, y_max, best):
    """construct_ei and its gradient from the P members' (μ, σ², ∇μ, ∇σ²) as ei_acquisition_grad composes them"""
    mu = np.stack([m[0] for m in moments])
    var = np.stack([np.maximum(m[1], 0.0) for m in moments])
    dmu = np.stack([m[2] for m in moments])
    dvar = np.stack([np.where(v > 0, m[3], 0.0) for m, v in zip(moments, var)])
    d, M = dmu.shape[1:]
    if y_max is None and best is None:
        return np.zeros(M), np.zeros((d, M))
    if best is None:
        return O.feas_prob_grad(mu, var, dmu, dvar, y_max)
    if y_max is None:
        return O.expected_improvement_lin_grad(coefs, mu, var, dmu, dvar, best)
    ei, dei = O.expected_improvement_lin_grad(coefs, mu, var, dmu, dvar, best)
    fp, dfp = O.feas_prob_grad(mu, var, dmu, dvar, y_max)
    return ei * fp, dei * fp + ei * dfp


def oracle_set(O, D, ns, P, mode, other=False):
    """(acq, ∇acq, bound on acq, bound on ∇acq, acq_ei's expectation): the mean over the samples, sample s on its first ns[s] points"""
    coefs = [1.0, 0.0][:P]
    y_max, best = mode_args(mode, P, D.best)
    acc, gacc, ba, bg, ei = 0.0, 0.0, 0.0, 0.0, 0.0
    S = len(ns)
    for s, n in enumerate(ns):
        mem = [D.member(O, n, s, p, other) for p in range(P)]
        a, g = compose(O, [m[2] for m in mem], coefs, y_max, best)
        tol = sum(m[1] for m in mem)
        acc, gacc = acc + a / S, gacc + g / S
        ba += 10 * tol / S
        bg += 100 * tol * (1 + np.abs(g).max()) / S
        mu, var = np.stack([m[2][0] for m in mem]), np.stack([np.maximum(m[2][1], 0.0) for m in mem])
        if best is None and y_max is None:
            e = np.zeros(M_)
        elif best is None:
            e = O.feas_prob(mu, var, y_max)
        else:
            e = O.expected_improvement_lin(coefs, mu, var, best) * (1.0 if y_max is None else O.feas_prob(mu, var, y_max))
        ei = ei + e / S
    return acc, gacc, ba, bg, ei


def build_grad_members(api, D, how, P, n0=N0, steps=STEPS):
    """gps[s][p]: `how` = "batch" the members of one ggp_fit_batch per output, "single" handles built one by one; then the same
    appends on every member, each on the path the Capacity rule predicts (block rows; the second step grows the storage)."""
    gps = [[None] * P for _ in range(S_)]
    try:
        for p in range(P):
            y, dY = D.Y[p], D.dY[p]
            hs = [hyper(s, p) for s in range(S_)]
            if how == "batch":
                row, _, st = api.ggp_fit_batch(D.X[:, :n0], y[:n0], dY[:, :n0], KERNEL, np.stack([h[0] for h in hs], axis=1),
                                               np.array([h[1] for h in hs]), np.array([h[2] for h in hs]), np.array([h[3] for h in hs]))
                for s in range(S_):
                    gps[s][p] = row[s]
                assert not st.any()
            else:
                for s in range(S_):
                    gps[s][p] = api.GradGP(D.X[:, :n0], y[:n0], dY[:, :n0], KERNEL)
                    gps[s][p].update(*hs[s])
            for s in range(S_):
                cap, n = GA.Capacity(n0 * (1 + D_)), n0
                for m in steps:
                    want = cap.path(n * (1 + D_), m * (1 + D_))
                    gps[s][p].append(D.X[:, n:n + m], y[n:n + m], dY[:, n:n + m])
                    n += m
                    assert api._append_path(gps[s][p]) == want == 1, (how, s, p, n, api._append_path(gps[s][p]), want)
    except BaseException:
        close_rows(gps)
        raise
    return gps


def close_rows(gps):
    for row in gps:
        for g in row:
            if g is not None:
                g.close()


def check_grad_set(api, O, D, gps, ns, mode, what, other=False, expect_set=True, loop=False):
    """acq_ei and acq_ei_grad_set over gps against the oracle; whether the set launches ran; optionally against the member loop"""
    P = len(gps[0])
    coefs = [1.0, 0.0][:P]
    y_max, best = mode_args(mode, P, D.best)
    acq_o, dacq_o, ba, bg, ei_o = oracle_set(O, D, ns, P, mode, other)
    no_set = os.environ.get("BOSS_NO_SET_PREDICT") == "1"
    if mode != "none":                                          # (boss_acq_ei has no variant without both terms)
        cand = api.Candidates(D.Xs)
        try:
            before = api._set_launches()
            ei, am, mx = api.acq_ei(gps, cand, coefs, y_max, best)
            after = api._set_launches()
        finally:
            cand.close()
        e = np.abs(ei - ei_o).max()
        print(f"{what} {mode}: acq_ei {e:.3e} (<= 1e-10)  set launches {before} -> {after}", flush=True)
        assert e <= 1e-10 and am == int(np.argmax(ei)), (what, mode, e)
        if expect_set is True:
            assert after[1] > before[1] or no_set, (what, "acq_ei did not take the set prediction")
        elif expect_set is False:
            assert after == before, (what, "acq_ei took the set prediction")
    before = api._set_grad_launches()
    acq, dacq = api.acq_ei_grad_set(gps, D.Xs, coefs, y_max, best)
    after = api._set_grad_launches()
    ea, eg = np.abs(acq - acq_o).max(), np.abs(dacq - dacq_o).max()
    print(f"{what} {mode}: |dacq| {ea:.3e} (<= {ba:.3e})  |dgrad| {eg:.3e} (<= {bg:.3e})  set grad launches {before} -> {after}", flush=True)
    assert ea <= ba and eg <= bg, (what, mode, ea, ba, eg, bg)
    if expect_set is True:
        assert after > before or no_set, (what, "acq_ei_grad_set did not take the set launches")
    elif expect_set is False:
        assert after == before, (what, "acq_ei_grad_set took the set launches")
    again = api.acq_ei_grad_set(gps, D.Xs, coefs, y_max, best)
    assert np.array_equal(again[0], acq) and np.array_equal(again[1], dacq), (what, mode, "two consecutive calls differ")
    if loop:
        res = [api.acq_ei_grad(row, D.Xs, coefs, y_max, best) for row in gps]
        acq_l, dacq_l = sum(r[0] for r in res) / len(res), sum(r[1] for r in res) / len(res)
        ea, eg = np.abs(acq - acq_l).max(), np.abs(dacq - dacq_l).max()
        print(f"{what} {mode}: set vs loop |dacq| {ea:.3e} (<= {2 * ba:.3e})  |dgrad| {eg:.3e} (<= {2 * bg:.3e})", flush=True)
        assert ea <= 2 * ba and eg <= 2 * bg, (what, mode, ea, eg)


def run_grad_set(api, O, how, P=1, modes=MODES):
    """Cases (a) and (b): the members, appended [1, 4] to 65 points of which 60 are head points (the second point split of the
    accumulation, points 33…64, straddles nhead), through the set calls in every mode; then re-updated with other hyper-parameters;
    then one member appended once more, after which the list is not uniform."""
    D = grad_data()
    gps = build_grad_members(api, D, how, P)
    try:
        assert all(g.n == NT and g.N == NT * (1 + D_) for row in gps for g in row)
        for mode in modes:                                      # (without both terms the acquisition is zero and nothing is launched)
            check_grad_set(api, O, D, gps, [NT] * S_, mode, f"{how} P={P}", loop=True, expect_set=True if mode != "none" else None)
        for s in range(S_):
            for p in range(P):
                gps[s][p].update(*hyper(s, p, other=True))
        check_grad_set(api, O, D, gps, [NT] * S_, "both", f"{how} P={P} re-updated", other=True, expect_set=None)
        for p in range(P):
            gps[0][p].append(D.X[:, NT:NT + 1], D.Y[p, NT:NT + 1], D.dY[p][:, NT:NT + 1])
        check_grad_set(api, O, D, gps, [NT + 1] + [NT] * (S_ - 1), "both", f"{how} P={P} one member longer", other=True, expect_set=False)
    finally:
        close_rows(gps)


def run_nhead_guard(api, O):
    """Case (c): the same 65 points and hyper-parameters in a handle created with all of them (nhead = 65) and in one created with
    60 and appended 5 (nhead = 60): equal N, Np, ld, npts, ldx, so only the nhead comparison keeps them off the set launches."""
    D = grad_data()
    fresh = api.GradGP(D.X[:, :NT], D.Y[0, :NT], D.dY[0][:, :NT], KERNEL)
    mixed = api.GradGP(D.X[:, :N0], D.Y[0, :N0], D.dY[0][:, :N0], KERNEL)
    try:
        h = hyper(0, 0)
        fresh.update(*h)
        mixed.update(*h)
        mixed.append(D.X[:, N0:NT], D.Y[0, N0:NT], D.dY[0][:, N0:NT])
        assert api._append_path(mixed) == GA.Capacity(N0 * (1 + D_)).path(N0 * (1 + D_), (NT - N0) * (1 + D_)) == 1
        assert fresh.N == mixed.N == NT * (1 + D_)
        post, tol, mo = D.member(O, NT, 0, 0)
        y_max, best = mode_args("both", 1, D.best)
        acq_o, dacq_o = compose(O, [mo], [1.0], y_max, best)
        ba, bg = 10 * tol, 100 * tol * (1 + np.abs(dacq_o).max())
        for pair, what in (([[fresh], [mixed]], "fresh, mixed"), ([[mixed], [fresh]], "mixed, fresh")):
            cand = api.Candidates(D.Xs)
            before = (api._set_launches(), api._set_grad_launches())
            ei, _, _ = api.acq_ei(pair, cand, [1.0], y_max, best)
            acq, dacq = api.acq_ei_grad_set(pair, D.Xs, [1.0], y_max, best)
            after = (api._set_launches(), api._set_grad_launches())
            cand.close()
            ea, eg = np.abs(acq - acq_o).max(), np.abs(dacq - dacq_o).max()
            print(f"nhead guard ({what}): acq_ei {np.abs(ei - acq_o).max():.3e}  |dacq| {ea:.3e} (<= {ba:.3e})  |dgrad| {eg:.3e} (<= {bg:.3e})"
                  f"  launches {before} -> {after}", flush=True)
            assert after == before, "handles of different nhead took the set launches"
            assert np.abs(ei - acq_o).max() <= 1e-10 and ea <= ba and eg <= bg, (what, ea, eg)
        for g, what in ((fresh, "fresh"), (mixed, "mixed")):    # every member's own contribution
            acq, dacq = api.acq_ei_grad([g], D.Xs, [1.0], y_max, best)
            assert np.abs(acq - acq_o).max() <= ba and np.abs(dacq - dacq_o).max() <= bg, what
        # the permutation is invisible: the two handles against each other, twice the single-handle bounds
        (mu_f, var_f), (mu_m, var_m) = fresh.predict(D.Xs), mixed.predict(D.Xs)
        e = (np.abs(mu_f - mu_m).max(), np.abs(var_f - var_m).max())
        print(f"nhead guard: predict fresh vs mixed mu {e[0]:.2e} var {e[1]:.2e}", flush=True)
        assert e[0] <= 2e-9 and e[1] <= 2e-9, e
        assert np.abs(mu_m - mo[0]).max() <= 1e-9 and np.abs(var_m - np.maximum(mo[1], 0)).max() <= 1e-9
        rf, rm = fresh.predict_grad(D.Xs), mixed.predict_grad(D.Xs)
        e = (np.abs(rf[0] - rm[0]).max(), np.abs(rf[1] - rm[1]).max(), np.abs(rf[2] - rm[2]).max() / (1 + np.abs(mo[2]).max()),
             np.abs(rf[3] - rm[3]).max() / (1 + np.abs(mo[3]).max()))
        print(f"nhead guard: predict_grad fresh vs mixed mu {e[0]:.2e} var {e[1]:.2e} dmu {e[2]:.2e} dvar {e[3]:.2e} (tol {tol:.2e})", flush=True)
        assert e[0] <= 2e-9 and e[1] <= 2e-9 and e[2] <= 20 * tol and e[3] <= 20 * tol, (e, tol)
    finally:
        fresh.close()
        mixed.close()


# ------------------------------------------------------------------------------------------ 1: gradient-observation sets
def test_appended_members_of_a_fitted_set(api, O):
    """(a) Members of ggp_fit_batch (d = 3, S = 3, 60 points = 240 rows), each appended [1, 4]: npts = 65, nhead = 60, 260 rows.  The
    accumulation splits the points in two, and the second split (33…64) holds head points and appended points, so one workgroup of
    aug_grad_accum_set_kernel runs both walk segments.  acq_ei 1e-10 (test_gpu_model_fit_batch.py:222); acq_ei_grad_set in all four
    construct_ei modes within the bounds of test_gpu_acq_grad_set.py:158-169, within twice those of the loop of acq_ei_grad, twice
    bit for bit; both launch counters rise.  Then every member re-updated (a re-factorisation in the mixed ordering), then one
    member one point longer: no set launches, same bounds."""
    run_grad_set(api, O, "batch")


def test_appended_handles_built_one_by_one(api, O):
    """(b) The same members from api.GradGP + update + the same appends: they never shared storage, and take the set launches."""
    run_grad_set(api, O, "single")


def test_appended_members_with_two_outputs(api, O):
    """P = 2: EI of output 0 × feasibility of output 1 over appended members of two ggp_fit_batch sets."""
    run_grad_set(api, O, "batch", P=2, modes=("both",))


def test_handles_of_different_nhead_stay_off_the_set_launches(api, O):
    """(c) predict_set_ok's nhead comparison, which alone separates these two handles; both orders of the pair."""
    run_nhead_guard(api, O)


# ------------------------------------------------------------------------------------------ 2: nonstationary sets
NS_N0, NS_N, NS_M = 250, 260, 70
_NS_CASES = {}


def ns_case(api, O, disc):
    """tests/test_gpu_ngp_grad_set.py's Case on ALL 260 points (S = 3, P = 2, per-sample prior means, Jacobians): the oracle's
    posteriors, moments and bounds, computed once per variant; its own never-appended handles are closed at once."""
    key = None if disc is None else tuple(disc)
    if key not in _NS_CASES:
        case = NG.Case(api, O, NS_N, NS_M, S=S_, P=2, discrete=disc, seed=5)
        case.close()
        case.gps = None
        _NS_CASES[key] = case
    return _NS_CASES[key]


def ns_member_arrays(case, s, p, a, b):
    """(λ, α, σ, m) of member (s, p) at the points a…b−1 from the case's closures (λ, α at the rounded points)"""
    X = case.X[:, a:b]
    Xr = X if case.disc is None else np.where(case.disc[:, None], np.rint(X), X)
    f_lam, _, f_amp, _, f_noise = case.lat[s][p]
    return NG.ev(f_lam, Xr).T, NG.ev(f_amp, Xr), NG.ev(f_noise, X), NG.ev(case.mean[s][p], X)


def build_ns_members(api, case, how, N0=NS_N0):
    S, P, d, N = case.S, case.P, case.d, case.N
    gps = [[None] * P for _ in range(S)]
    try:
        for p in range(P):
            arr = [ns_member_arrays(case, s, p, 0, N0) for s in range(S)]
            if how == "batch":
                row, _, st = api.ngp_fit_batch(case.X[:, :N0], case.Y[p, :N0], np.asfortranarray(np.stack([a[0] for a in arr], axis=2)),
                                               np.asfortranarray(np.stack([a[1] for a in arr], axis=1)),
                                               np.asfortranarray(np.stack([a[2] for a in arr], axis=1)), np.stack([a[3] for a in arr]), case.disc)
                for s in range(S):
                    gps[s][p] = row[s]
                assert not st.any()
            else:
                for s in range(S):
                    gps[s][p] = api.GibbsGP(case.X[:, :N0], case.Y[p, :N0], case.disc)
                    gps[s][p].update(*arr[s])
            for s in range(S):
                want = _NGA().Capacity(N0).path(N0, N - N0)
                gps[s][p].append(case.X[:, N0:N], case.Y[p, N0:N], *ns_member_arrays(case, s, p, N0, N))
                assert api._append_path(gps[s][p]) == want == 1, (how, s, p, api._append_path(gps[s][p]), want)
    except BaseException:
        close_rows(gps)
        raise
    return gps


def _NGA():
    import test_gpu_ngp_append_track as T
    return T


def run_ns_set(api, O, how, disc=None):
    """Members on 250 points appended 10 (256 rows of storage grow to 512: block rows after a growth), against the oracle on all 260:
    ngp_predict_set, ngp_predict_grad_set, ngp_acq_ei_grad_set in all four modes; counters; twice bit for bit; then one member one
    observation longer."""
    case = copy.copy(ns_case(api, O, disc))
    case.gps = build_ns_members(api, case, how)
    what = f"nonstationary {how}" + (" discrete" if disc is not None else "")
    no_set = os.environ.get("BOSS_NO_SET_PREDICT") == "1"
    try:
        flat = case.flat()
        assert all(g.N == NS_N for g in flat)
        before = api._set_launches()
        mu, var = api.ngp_predict_set(flat, case.Xs, case.lamS, case.ampS, case.ms)
        assert api._set_launches()[1] > before[1] or no_set, "ngp_predict_set over appended members did not take the set prediction"
        for i in range(case.n):
            tol = case.tol[i // case.P, i % case.P]
            mu_o, var_o = case.full[i][0], np.maximum(case.full[i][1], 0.0)
            e, b = (np.abs(mu[i] - mu_o).max(), np.abs(var[i] - var_o).max()), (tol * (1 + np.abs(mu_o).max()), tol * case.ampS[:, i].max() ** 2)
            print(f"{what} predict_set member {i}: mu {e[0]:.2e} (<= {b[0]:.2e})  var {e[1]:.2e} (<= {b[1]:.2e})", flush=True)
            assert e[0] <= b[0] and e[1] <= b[1], (what, i, e, b)
        again = api.ngp_predict_set(flat, case.Xs, case.lamS, case.ampS, case.ms)
        assert np.array_equal(again[0], mu) and np.array_equal(again[1], var)
        NG.check_case(api, O, case, what)                       # predict_grad_set, the four acquisition modes, the set-grad counter
        r = [NG.predict_grad_set(api, case) for _ in range(2)]
        a = [case.device_acq(api, O, "both") for _ in range(2)]
        assert all(np.array_equal(x, y) for x, y in zip(r[0], r[1])) and all(np.array_equal(x, y) for x, y in zip(a[0], a[1]))
        # one unequal append: member (0, 0) gets one more observation; the calls go member by member
        rng = np.random.default_rng(77)
        x = rng.uniform(0.1, 0.9, (case.d, 1)) * (np.where(case.disc, 3.0, 1.0)[:, None] if case.disc is not None else 1.0)
        y = np.array([float(np.sin(3 * x).sum())])
        xr = x if case.disc is None else np.where(case.disc[:, None], np.rint(x), x)
        f_lam, _, f_amp, _, f_noise = case.lat[0][0]
        new = (NG.ev(f_lam, xr).T, NG.ev(f_amp, xr), NG.ev(f_noise, x), NG.ev(case.mean[0][0], x))
        case.gps[0][0].append(x, y, *new)
        lam0, amp0, noi0, m0 = ns_member_arrays(case, 0, 0, 0, NS_N)
        post = O.nonstationary_fit(np.hstack([case.X, x]), np.concatenate([case.Y[0], y]), np.hstack([lam0, new[0]]),
                                   np.concatenate([amp0, new[1]]), np.concatenate([noi0, new[2]]), mean=np.concatenate([m0, new[3]]),
                                   discrete=case.disc)
        longer = copy.copy(case)
        longer.tol, longer.full = case.tol.copy(), list(case.full)
        longer.tol[0, 0] = max(1e-9, np.linalg.cond(post.L @ post.L.T) * (NS_N + 1) * 2.0 ** -53 * 8)
        longer.full[0] = O.nonstationary_mean_and_var_grad(post, case.Xs, case.lamS[:, :, 0], case.ampS[:, 0], case.Dl[:, :, :, 0],
                                                           case.Da[:, :, 0], case.ms[0], case.mg[0])
        before = (api._set_launches(), api._set_grad_launches())
        NG.assert_members(longer, NG.predict_grad_set(api, longer), longer.full, what + " one member longer")
        NG.assert_acq(longer, O, longer.device_acq(api, O, "both"), "both", what + " one member longer")
        mu, var = api.ngp_predict_set(longer.flat(), case.Xs, case.lamS, case.ampS, case.ms)
        assert (api._set_launches(), api._set_grad_launches()) == before, "a list with one longer member took the set launches"
        assert np.abs(mu[0] - longer.full[0][0]).max() <= longer.tol[0, 0] * (1 + np.abs(longer.full[0][0]).max())
    finally:
        close_rows(case.gps)


@pytest.mark.parametrize("how,disc", [("batch", None), ("single", None), ("batch", [False, True, False])])
def test_appended_nonstationary_members(api, O, how, disc):
    """Members of ngp_fit_batch / handles built one by one (d = 3, S = 3, P = 2, per-sample prior means; once with a discrete
    dimension) on 250 points, appended 10, against the oracle on all 260 with the bounds of tests/test_gpu_ngp_grad_set.py:8-11."""
    run_ns_set(api, O, how, disc)


def run_ns_latents(api, O):
    """Resident latents: tests/test_gpu_nlat.py's Members on 250 points, every member appended the same 10 points with the latent
    values lat.eval gives there; each _lat set call equals its array twin bit for bit on boss_nlat_eval's arrays, on the set launches."""
    import test_gpu_nlat as NL
    # seed 6: with the oracle cond(K) <= 6.7e4 on all 260 points and σ² >= 9.9e-5 at the candidates.  The Gibbs kernel's amplitude
    # factor ((α(x) + α(y)) / 2)² is not positive semi-definite, and under other seeds one member's matrix is not positive definite
    # at 260 points (seed 0) or a variance falls to −1.7e-4 (seed 3) — in the oracle as on the device.
    c = NL.Members(api, O, N=NS_N0, M=33, S=S_, P=2, seed=6)
    try:
        Xn = np.random.default_rng(913).uniform(0, 1, (c.d, NS_N - NS_N0))
        Yn = np.stack([np.sin(3 * Xn).sum(0), Xn[0] - Xn[1] + 0.2 * np.cos(4 * Xn[2])])
        for s in range(c.S):
            for p in range(c.P):
                lam, amp, noi, _, _ = c.lats[s][p].eval(Xn, jac=False, noise=True)
                c.gps[s][p].append(Xn, Yn[p], lam, amp, noi)
                assert api._append_path(c.gps[s][p]) == 1 and c.gps[s][p].N == NS_N
        NL.check_set_calls(api, c, "appended members", expect_set=None if os.environ.get("BOSS_NO_SET_PREDICT") == "1" else True)
    finally:
        c.close()


def test_appended_nonstationary_members_with_resident_latents(api, O):
    """The rule tests/test_gpu_nlat.py:10 states for fresh handles, on appended members: _lat calls bit for bit their array twins."""
    run_ns_latents(api, O)


# ------------------------------------------------------------------------------------------ 3: poisoned allocations
CHILD_POISON = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
entry.build()
from boss_jl_amd import api
from oracle import gp_oracle as O
import test_gpu_appended_sets as T
T.%(call)s
print("RES ok")
'''


def poisoned(call, timeout):
    code = CHILD_POISON % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "call": call}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BOSS_POISON_ALLOC="1"), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "RES ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_gradient_set_on_poisoned_allocations(api):
    """Case (a) once more with every fresh device block filled with NaN patterns (BOSS_POISON_ALLOC=1, a child process): the arrays
    gp_grow and ggp_grow_points hand out uninitialised (the second append grows the storage) and the set kernels' scratch."""
    poisoned('run_grad_set(api, O, "batch")', 300)


def test_nonstationary_set_on_poisoned_allocations(api):
    """The nonstationary set case (members of ngp_fit_batch, the append grows the storage) on poisoned allocations."""
    poisoned('run_ns_set(api, O, "batch")', 300)
