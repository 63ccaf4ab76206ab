"""boss_ngp_predict_grad_set / boss_ngp_acq_ei_grad_set: moments with candidate gradients of a list of nonstationary posteriors, and
the acquisition with its gradient averaged over the S samples of a Bayesian-inference fit, in one device call (pytest -m gpu).

Expectation: per member the oracle's nonstationary_fit + nonstationary_mean_and_var_grad (finite-difference checked in
tests/test_oracle_crosscheck.py), composed as ei_acquisition_grad composes expected_improvement_lin_grad and feas_prob_grad, and
averaged over s (src/acquisitions/expected_improvement.jl:87-90 under optimization.jl:89-118).

Tolerances: the rule of tests/test_gpu_parity.py:2066-2083 per member, tol = max(1e-9, cond(K) N 2^-53 8):
|Δμ| <= tol (1 + max|μ|), |Δσ²| <= tol max α*², |Δ∇| <= 10 tol (1 + max|∇|); acquisition |Δacq| <= 10 tol, |Δ∇acq| <= 100 tol
(1 + max|∇acq|).  A sample's acquisition reads the moments of its P members, so its tol is the sum of theirs (triangle inequality);
the set is held to the mean over s of its samples' bounds, as tests/test_gpu_acq_grad_set.py::run_grad_model does.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("both", "best_only", "cons_only", "none")


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


def latents(d, sl, sa):
    """The latent models of tests/test_gpu_parity.py:2046-2054 scaled by (sl, sa): closures and analytic Jacobians."""
    w = np.linspace(0.5, 1.5, d)
    k = np.arange(1, d + 1)
    f_lam = lambda x: sl * (0.3 + 0.4 * np.asarray(x) ** 2 + 0.05 * k + 0.1 * np.sin(w @ np.asarray(x)))              # noqa: E731
    J_lam = lambda x: sl * (np.diag(0.8 * np.asarray(x)) + 0.1 * np.cos(w @ np.asarray(x)) * np.tile(w, (d, 1)))      # noqa: E731
    f_amp = lambda x: sa * (1.0 + 0.4 * np.sin(3 * x[0]) + 0.1 * x[-1])                                                # noqa: E731

    def J_amp(x):
        g = np.zeros(d)
        g[0] += 1.2 * np.cos(3 * x[0])
        g[-1] += 0.1
        return sa * g
    f_noise = lambda x: 0.05 + 0.02 * x[0]                                                                             # noqa: E731
    return f_lam, J_lam, f_amp, J_amp, f_noise


def ev(f, Z):
    return np.array([f(Z[:, j]) for j in range(Z.shape[1])])


class Case:
    """S samples × P outputs of a nonstationary model on N points: per output the members of one ngp_fit_batch, every member with
    its own scaled latent models and prior mean m(x) = c + gᵀx; the oracle's per-member moments and gradients at M candidates in
    [0.05, 0.95]^d (×3 in the discrete dimensions, so that rounding matters), with and without the latent Jacobians."""

    def __init__(self, api, O, N, M, d=3, S=4, P=2, discrete=None, seed=0, N_alt=None):
        rng = np.random.default_rng(7000 + 13 * N + M + 101 * d + seed)
        self.N, self.M, self.d, self.S, self.P, self.n = N, M, d, S, P, S * P
        self.disc = None if discrete is None else np.asarray(discrete, bool)
        scale = np.where(self.disc, 3.0, 1.0)[:, None] if self.disc is not None else 1.0
        X = rng.uniform(0, 1, (d, N)) * scale
        Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)) * scale)
        rnd = lambda Z: Z if self.disc is None else np.where(self.disc[:, None], np.rint(Z), Z)                        # noqa: E731
        Xr, Xsr = rnd(X), rnd(Xs)
        Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1 % d] + 0.2 * np.cos(4 * X[2 % d])])[:P]
        self.X, self.Y, self.Xs = X, Y, Xs
        sl, sa = rng.uniform(0.8, 1.4, (S, P)), rng.uniform(0.8, 1.3, (S, P))
        c, gr = rng.uniform(-0.2, 0.2, (S, P)), rng.uniform(-0.2, 0.2, (S, P, d))
        self.mask = np.ones(M, bool)
        self.mask[::7] = False
        self.coefs = [1.0, 0.2][:P]
        n = self.n
        self.lamS, self.ampS = np.empty((d, M, n), order="F"), np.empty((M, n), order="F")
        self.Dl, self.Da = np.empty((d, d, M, n), order="F"), np.empty((d, M, n), order="F")
        self.ms, self.mg = np.empty((n, M)), np.empty((n, d, M))
        self.lat = [[latents(d, sl[s, p], sa[s, p]) for p in range(P)] for s in range(S)]
        self.mean = [[(lambda x, s=s, p=p: float(c[s, p] + gr[s, p] @ np.asarray(x))) for p in range(P)] for s in range(S)]
        self.gps = [[None] * P for _ in range(S)]
        self.posts = [[None] * P for _ in range(S)]
        self.tol = np.empty((S, P))
        self.full, self.const = [None] * n, [None] * n
        # members s >= S_alt of an N_alt case are fitted on the first N_alt points only (a list of two shapes)
        for p in range(P):
            groups = [(range(S), N)] if N_alt is None else [(range(S // 2), N), (range(S // 2, S), N_alt)]
            for members, Nn in groups:
                members = list(members)
                lamX = np.empty((d, Nn, len(members)), order="F")
                ampX, noiX = np.empty((Nn, len(members)), order="F"), np.empty((Nn, len(members)), order="F")
                mX = np.empty((len(members), Nn))
                for q, s in enumerate(members):
                    f_lam, _, f_amp, _, f_noise = self.lat[s][p]
                    lamX[:, :, q], ampX[:, q], noiX[:, q] = ev(f_lam, Xr[:, :Nn]).T, ev(f_amp, Xr[:, :Nn]), ev(f_noise, X[:, :Nn])
                    mX[q] = c[s, p] + gr[s, p] @ X[:, :Nn]
                gp, _, st = api.ngp_fit_batch(X[:, :Nn], Y[p, :Nn], lamX, ampX, noiX, mX, self.disc)
                assert not st.any()
                for q, s in enumerate(members):
                    self.gps[s][p] = gp[q]
                    post = O.nonstationary_fit(X[:, :Nn], Y[p, :Nn], lamX[:, :, q], ampX[:, q], noiX[:, q], mean=mX[q], discrete=self.disc)
                    self.posts[s][p] = post
                    self.tol[s, p] = max(1e-9, np.linalg.cond(post.L @ post.L.T) * Nn * 2.0 ** -53 * 8)
            for s in range(S):
                i = p + P * s
                f_lam, J_lam, f_amp, J_amp, _ = self.lat[s][p]
                self.lamS[:, :, i], self.ampS[:, i] = ev(f_lam, Xsr).T, ev(f_amp, Xsr)
                self.Dl[:, :, :, i] = np.stack([J_lam(Xsr[:, j]) for j in range(M)], axis=2)
                self.Da[:, :, i] = np.stack([J_amp(Xsr[:, j]) for j in range(M)], axis=1)
                if self.disc is not None:
                    self.Dl[:, self.disc, :, i] = 0.0
                    self.Da[self.disc, :, i] = 0.0
                self.ms[i] = c[s, p] + gr[s, p] @ Xs
                self.mg[i] = np.repeat(gr[s, p][:, None], M, axis=1)
                post = self.posts[s][p]
                self.full[i] = O.nonstationary_mean_and_var_grad(post, Xs, self.lamS[:, :, i], self.ampS[:, i], self.Dl[:, :, :, i],
                                                                 self.Da[:, :, i], self.ms[i], self.mg[i])
                self.const[i] = O.nonstationary_mean_and_var_grad(post, Xs, self.lamS[:, :, i], self.ampS[:, i], None, None, self.ms[i],
                                                                  self.mg[i])

    def flat(self):
        return [self.gps[s][p] for s in range(self.S) for p in range(self.P)]

    def args(self, O, mode):
        y_max = [np.inf, 0.3][:self.P] if mode in ("both", "cons_only") else None
        b = O.best_so_far(self.coefs, self.Y, [np.inf, 0.3][:self.P]) if mode in ("both", "best_only") else None
        return y_max, b

    def oracle_acq(self, O, mode, moments=None):
        """(acq, dacq, bound_acq, bound_grad): ei_acquisition_grad's composition on the members' oracle moments, mean over s"""
        moments = self.full if moments is None else moments
        y_max, b = self.args(O, mode)
        S, P, d, M = self.S, self.P, self.d, self.M
        acc, gacc, ba, bg = np.zeros(M), np.zeros((d, M)), 0.0, 0.0
        for s in range(S):
            mo = [moments[p + P * s] for p in range(P)]
            mu = np.stack([m[0] for m in mo])
            var = np.stack([np.maximum(m[1], 0.0) for m in mo])
            dmu = np.stack([m[2] for m in mo])
            dvar = np.stack([np.where(v > 0, m[3], 0.0) for m, v in zip(mo, var)])
            if y_max is None and b is None:
                a, g = np.zeros(M), np.zeros((d, M))
            elif b is None:
                a, g = O.feas_prob_grad(mu, var, dmu, dvar, y_max)
            elif y_max is None:
                a, g = O.expected_improvement_lin_grad(self.coefs, mu, var, dmu, dvar, b)
            else:
                ei, dei = O.expected_improvement_lin_grad(self.coefs, mu, var, dmu, dvar, b)
                fp, dfp = O.feas_prob_grad(mu, var, dmu, dvar, y_max)
                a, g = ei * fp, dei * fp + ei * dfp
            a, g = np.where(self.mask, a, 0.0), np.where(self.mask[None, :], g, 0.0)
            tol = self.tol[s].sum()
            acc, gacc = acc + a, gacc + g
            ba += 10 * tol / S
            bg += 100 * tol * (1 + np.abs(g).max()) / S
        return acc / S, gacc / S, ba, bg

    def device_acq(self, api, O, mode, jac=True):
        y_max, b = self.args(O, mode)
        return api.ngp_acq_ei_grad_set(self.gps, self.Xs, self.lamS, self.ampS, self.Dl if jac else None, self.Da if jac else None,
                                       self.coefs, y_max, b, self.mask, self.ms, self.mg)

    def close(self):
        for row in self.gps:
            for g in row:
                g.close()


def assert_members(case, res, moments, what, factor=1.0):
    mu, var, dmu, dvar = res
    for i in range(case.n):
        tol = factor * case.tol[i // case.P, i % case.P]
        mu_o, var_o, dmu_o, dvar_o = moments[i]
        errs = (np.abs(mu[i] - mu_o).max(), np.abs(var[i] - np.maximum(var_o, 0.0)).max(), np.abs(dmu[i] - dmu_o).max(),
                np.abs(dvar[i] - dvar_o).max())
        bounds = (tol * (1 + np.abs(mu_o).max()), tol * case.ampS[:, i].max() ** 2, 10 * tol * (1 + np.abs(dmu_o).max()),
                  10 * tol * (1 + np.abs(dvar_o).max()))
        print(f"{what} member {i}: " + "  ".join(f"{e:.2e} (<= {b:.2e})" for e, b in zip(errs, bounds)), flush=True)
        assert all(e <= b for e, b in zip(errs, bounds)), (what, i, errs, bounds)


def assert_acq(case, O, res, mode, what, moments=None, factor=1.0):
    acq, dacq = res
    acq_o, dacq_o, ba, bg = case.oracle_acq(O, mode, moments)
    ea, eg = np.abs(acq - acq_o).max(), np.abs(dacq - dacq_o).max()
    print(f"{what} {mode}: |dacq| {ea:.3e} (<= {factor * ba:.3e})  |dgrad| {eg:.3e} (<= {factor * bg:.3e})", flush=True)
    assert ea <= factor * ba and eg <= factor * bg, (what, mode, ea, ba, eg, bg)
    assert np.all(acq[~case.mask] == 0.0) and np.all(dacq[:, ~case.mask] == 0.0), what


def predict_grad_set(api, case, jac=True):
    return api.ngp_predict_grad_set(case.flat(), case.Xs, case.lamS, case.ampS, case.Dl if jac else None, case.Da if jac else None,
                                    case.ms, case.mg)


def check_case(api, O, case, what, expect_set=True):
    before = api._set_grad_launches()
    assert_members(case, predict_grad_set(api, case), case.full, what)
    for mode in MODES:
        assert_acq(case, O, case.device_acq(api, O, mode), mode, what)
    if expect_set:
        assert api._set_grad_launches() > before or os.environ.get("BOSS_NO_SET_PREDICT") == "1"
    else:
        assert api._set_grad_launches() == before


@pytest.fixture(scope="module")
def small(api, O):
    """the case most tests share: built once, left unchanged"""
    case = Case(api, O, 260, 70)
    yield case
    case.close()


# ------------------------------------------------------------------------------------------ 1: members against the oracle
@pytest.mark.parametrize("N,M", [(N, M) for N in (260, 1030) for M in (70, 224)])
def test_members_against_the_oracle(api, O, N, M):
    """Members of ngp_fit_batch (d = 3, S = 4, P = 2; two and five 256-row blocks with ragged ends, three tiles with a partial
    last one and seven tiles), Jacobians and per-member prior means with gradients: boss_ngp_predict_grad_set per member and
    boss_ngp_acq_ei_grad_set in all four construct_ei variants with a mask; the set launches ran."""
    case = Case(api, O, N, M)
    try:
        assert min(m[1].min() for m in case.full) >= 7e-5     # (no candidate is clipped or poisoned)
        check_case(api, O, case, f"N={N} M={M}")
    finally:
        case.close()


def test_members_at_the_dimension_limit(api, O):
    """d = 16 (GIBBS_GRAD_MAX_D), N = 150, M = 33, S = 3, P = 1."""
    case = Case(api, O, 150, 33, d=16, S=3, P=1)
    try:
        check_case(api, O, case, "d=16")
    finally:
        case.close()


# ------------------------------------------------------------------------------------------ 2: the Jacobian fold
def test_the_jacobian_fold_is_exercised(api, O, small):
    """On the oracle alone the gradients without Jacobians differ from the full ones by >= 1000 bounds (the pattern of
    tests/test_gpu_parity.py:2114); the device without Jacobians meets the constant-latent oracle, with them the full one."""
    for i in range(small.n):
        tol = small.tol[i // small.P, i % small.P]
        for k in (2, 3):
            assert np.abs(small.full[i][k] - small.const[i][k]).max() >= 1000 * 10 * tol * (1 + np.abs(small.full[i][k]).max()), (i, k)
    assert_members(small, predict_grad_set(api, small, jac=False), small.const, "constant latents")
    assert_members(small, predict_grad_set(api, small, jac=True), small.full, "with Jacobians")
    assert_acq(small, O, small.device_acq(api, O, "both", jac=False), "both", "constant latents", small.const)
    assert_acq(small, O, small.device_acq(api, O, "both", jac=True), "both", "with Jacobians")


# ------------------------------------------------------------------------------------------ 3: set against loop
def loop(api, O, case, mode, samples=None):
    """the member-by-member public path: GibbsGP.predict_grad, acq_ei_grad_moments per sample, host mean"""
    y_max, b = case.args(O, mode)
    samples = range(case.S) if samples is None else samples
    res = []
    for s in samples:
        mo = []
        for p in range(case.P):
            i = p + case.P * s
            mo.append(case.gps[s][p].predict_grad(case.Xs, case.lamS[:, :, i], case.ampS[:, i], case.Dl[:, :, :, i], case.Da[:, :, i],
                                                  case.ms[i], case.mg[i]))
        res.append(api.acq_ei_grad_moments(np.stack([m[0] for m in mo]), np.stack([m[1] for m in mo]), np.stack([m[2] for m in mo]),
                                           np.stack([m[3] for m in mo]), case.coefs, y_max, b, case.mask))
    return sum(r[0] for r in res) / len(res), sum(r[1] for r in res) / len(res)


def test_set_equals_the_loop(api, O, small):
    """Against GibbsGP.predict_grad + acq_ei_grad_moments + host mean, within twice the bounds (two results that each meet them)."""
    for mode in MODES:
        acq, dacq = small.device_acq(api, O, mode)
        acq_l, dacq_l = loop(api, O, small, mode)
        _, dacq_o, ba, bg = small.oracle_acq(O, mode)
        ea, eg = np.abs(acq - acq_l).max(), np.abs(dacq - dacq_l).max()
        print(f"set vs loop {mode}: {ea:.3e} (<= {2 * ba:.3e})  {eg:.3e} (<= {2 * bg:.3e})", flush=True)
        assert ea <= 2 * ba and eg <= 2 * bg, (mode, ea, eg)


# ------------------------------------------------------------------------------------------ 4: determinism and path
def test_repeated_calls_are_bit_identical(api, O, small):
    a = [small.device_acq(api, O, "both") for _ in range(3)]
    m = [predict_grad_set(api, small) for _ in range(2)]
    assert all(np.array_equal(a[0][0], r[0]) and np.array_equal(a[0][1], r[1]) for r in a[1:])
    assert all(np.array_equal(x, y) for x, y in zip(m[0], m[1]))


def test_members_of_two_shapes_go_member_by_member(api, O):
    case = Case(api, O, 300, 70, N_alt=260)
    try:
        check_case(api, O, case, "N = 300 and 260", expect_set=False)
    finally:
        case.close()


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from boss_jl_amd import api
from oracle import gp_oracle as O
import test_gpu_ngp_grad_set as T
case = T.Case(api, O, 260, 70)
T.check_case(api, O, case, "BOSS_NO_SET_PREDICT=1")
assert api._set_grad_launches() == 0, api._set_grad_launches()
case.close()
print("CHILD_OK")
'''


def test_no_set_predict_switch_goes_member_by_member(api):
    env = dict(os.environ, BOSS_NO_SET_PREDICT="1")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------ 5: discrete dimension
def test_discrete_dimension_has_a_zero_gradient_row(api, O):
    case = Case(api, O, 260, 70, discrete=[False, True, False])
    try:
        check_case(api, O, case, "discrete")
        _, _, dmu, dvar = predict_grad_set(api, case)
        assert np.all(dmu[:, 1, :] == case.mg[:, 1, :]) and np.all(dvar[:, 1, :] == 0.0)
        case.mg[:] = 0.0
        acq, dacq = case.device_acq(api, O, "both")
        assert np.all(dacq[1] == 0.0) and np.abs(dacq[0]).max() > 0
    finally:
        case.close()


# ------------------------------------------------------------------------------------------ 6: S = 1
def test_one_sample_two_outputs(api, O):
    """S = 1, P = 2: the MAP case in one call equals acq_ei_grad_moments on two predict_grad results within the bounds."""
    case = Case(api, O, 260, 70, S=1, P=2)
    try:
        for mode in MODES:
            acq, dacq = case.device_acq(api, O, mode)
            assert_acq(case, O, (acq, dacq), mode, "S=1")
            acq_l, dacq_l = loop(api, O, case, mode)
            _, _, ba, bg = case.oracle_acq(O, mode)
            assert np.abs(acq - acq_l).max() <= 2 * ba and np.abs(dacq - dacq_l).max() <= 2 * bg
    finally:
        case.close()


# ------------------------------------------------------------------------------------------ 7: errors
def test_errors_leave_the_handles_usable(api, O, small):
    c = small

    def valid():
        assert_members(c, predict_grad_set(api, c), c.full, "after an error")
        assert_acq(c, O, c.device_acq(api, O, "both"), "both", "after an error")

    def both_calls(gps_rows, lamS=None, code=None):
        lamS = c.lamS if lamS is None else lamS
        flat = [g for row in gps_rows for g in row]
        with pytest.raises(api.BossError) as e:
            api.ngp_predict_grad_set(flat, c.Xs, lamS, c.ampS, c.Dl, c.Da, c.ms, c.mg)
        assert e.value.code == code, e.value
        with pytest.raises(api.BossError) as e:
            api.ngp_acq_ei_grad_set(gps_rows, c.Xs, lamS, c.ampS, c.Dl, c.Da, c.coefs, None, 0.1, c.mask, c.ms, c.mg)
        assert e.value.code == code, e.value
        valid()

    def swapped(g):
        rows = [list(r) for r in c.gps]
        rows[1][0] = g
        return rows
    # a plain handle in the list
    plain = api.GP(c.X, c.Y[0], "sqexp")
    plain.update(np.full(c.d, 0.5), 1.0, 0.1)
    both_calls(swapped(plain), code=api.BOSS_E_INVALID)
    plain.close()
    # an unfitted member: the second set of this ngp_fit_batch is invalid
    f_lam, _, f_amp, _, f_noise = c.lat[0][0]
    lamX = np.asfortranarray(np.repeat(ev(f_lam, c.X).T[:, :, None], 2, axis=2))
    ampX = np.asfortranarray(np.repeat(ev(f_amp, c.X)[:, None], 2, axis=1))
    noiX = np.asfortranarray(np.repeat(ev(f_noise, c.X)[:, None], 2, axis=1))
    ampX[:, 1] = -1.0
    two, _, st = api.ngp_fit_batch(c.X, c.Y[0], lamX, ampX, noiX)
    assert st[0] == 0 and st[1] != 0
    both_calls(swapped(two[1]), code=api.BOSS_E_NOT_FITTED)
    for g in two:
        g.close()
    # x_dim mismatch
    g2 = api.GibbsGP(c.X[:2], c.Y[0])
    g2.update(np.full((2, c.N), 0.5), np.full(c.N, 1.0), np.full(c.N, 0.1))
    both_calls(swapped(g2), code=api.BOSS_E_INVALID)
    g2.close()
    # a non-positive lengthscale at a candidate
    bad = c.lamS.copy(order="F")
    bad[1, 5, 3] = 0.0
    both_calls(c.gps, lamS=bad, code=api.BOSS_E_INVALID)


def test_negative_variance_fails_with_the_members_index(api):
    """The construction of tests/test_gpu_model_fit_batch.py::test_nonstationary_set_prediction_domain_error: the set call raises
    what the offending member's own predict_grad raises, with its bad_index; the healthy member alone is fine afterwards."""
    X = np.arange(0.0, 400.0, 10.0)[None, :]
    y = np.sin(X[0])
    N = X.shape[1]
    lam = np.asfortranarray(np.full((1, N, 3), 3.0))
    amp = np.asfortranarray(np.stack([np.full(N, 1.0), np.full(N, 1e5), np.full(N, 1e5)], axis=1))
    noi = np.asfortranarray(np.stack([np.full(N, 0.1), np.full(N, 1e-4), np.full(N, 1e-4)], axis=1))
    gps, _, st = api.ngp_fit_batch(X, y, lam, amp, noi)
    assert not st.any()
    ref = gps[0].predict_grad(X, lam[:, :, 0], amp[:, 0])
    with pytest.raises(api.DomainError) as e1:
        gps[1].predict_grad(X, lam[:, :, 1], amp[:, 1])
    with pytest.raises(api.DomainError) as e:
        api.ngp_predict_grad_set(gps, X, lam, amp)
    assert e.value.code == api.BOSS_E_NEG_VAR and e.value.bad_index == e1.value.bad_index and 0 <= e.value.bad_index < N
    res = api.ngp_predict_grad_set(gps[:1] + gps[:1], X, lam[:, :, [0, 0]], amp[:, [0, 0]])
    for k in range(4):
        assert np.allclose(res[k][1], ref[k], rtol=0, atol=1e-9 * (1 + np.abs(ref[k]).max()))
    for g in gps:
        g.close()


# ------------------------------------------------------------------------------------------ 8: host mirror
def test_host_mirror(api, O):
    """B.nonstationary_acq_ei_grad_batch on nonstationary_model_posterior_batch output: with analytic Jacobians within the bounds of
    the oracle; with central differences within rtol 1e-5 / atol 1e-8 of that (tests/test_oracle_crosscheck.py:142-149)."""
    import boss_jl_amd as B
    from boss_jl_amd.problem import ExperimentData
    case = Case(api, O, 260, 70)
    try:
        S, P = case.S, case.P
        models = [B.HipNonstationaryGP([case.lat[s][p][0] for p in range(P)], [case.lat[s][p][2] for p in range(P)],
                                       [case.lat[s][p][4] for p in range(P)], mean=[case.mean[s][p] for p in range(P)]) for s in range(S)]
        posts = B.nonstationary_model_posterior_batch(models, ExperimentData(case.X, case.Y))
        try:
            y_max, b = case.args(O, "both")
            mg = case.mg.reshape(S, P, case.d, case.M)
            lj = [[case.lat[s][p][1] for p in range(P)] for s in range(S)]
            aj = [[case.lat[s][p][3] for p in range(P)] for s in range(S)]
            res = B.nonstationary_acq_ei_grad_batch(posts, case.Xs, case.coefs, y_max, b, case.mask, lj, aj, mg)
            assert_acq(case, O, res, "both", "host mirror")
            fd = B.nonstationary_acq_ei_grad_batch(posts, case.Xs, case.coefs, y_max, b, case.mask, None, None, mg)
            assert np.allclose(fd[0], res[0], rtol=1e-5, atol=1e-8) and np.allclose(fd[1], res[1], rtol=1e-5, atol=1e-8)
        finally:
            for row in posts:
                for p_ in row:
                    p_.close()
    finally:
        case.close()
