"""boss_acq_ei_grad_set: the acquisition and its gradient w.r.t. the candidates, averaged over the S hyper-parameter samples of a
Bayesian-inference fit in one device call (pytest -m gpu).

The reference averages the acquisition over the samples (/root/reference/src/acquisitions/expected_improvement.jl:87-90) and
OptimizationAM differentiates that average (/root/reference/src/acquisition_maximizers/optimization.jl:36,89-118).  The expectation
is the mean over s of the oracle's single-sample gradient (checked against finite differences in tests/test_acq_grad_set_host.py).

Tolerances are the ones boss_acq_ei_grad is already held to (tests/test_gpu_parity.py:1073-1075): |Δacq| <= 1e-11,
|Δ∇acq| <= 1e-9 (1 + max|∇acq_oracle|), exact zeros under the mask — the mean of S members that each meet a bound meets it too.
Gradient-observation members: tests/test_gpu_parity.py:1695,1706-1707, tol = max(1e-9, cond(K) rows 2^-53 8) per member,
|Δacq| <= 10 tol, |Δ∇acq| <= 100 tol (1 + max|∇acq_oracle|); the set is held to the mean of its members' bounds.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S_, P_, D_ = 5, 2, 3
MODES = ("both", "best_only", "cons_only", "none")
PLAIN_CASES = [(N, M, k) for N in (260, 1030) for M in (70, 224) for k in ("matern52", "sqexp")]
GRAD_CASES = [(n, M) for n in (60, 65) for M in (70, 224)]            # n (1 + d) = 240, 260 rows


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


# ------------------------------------------------------------------------------------------ cases
class Plain:
    """S samples × P outputs of a plain model on N points: members of one fit_batch per output, per-sample prior means
    m_sp(x) = c_sp + g_spᵀx with their gradients, the oracle posteriors, candidates partly outside [0, 1]^d."""

    def __init__(self, api, O, N, M, kernel, S=S_, P=P_, d=D_, seed=0, bad_sample=None):
        rng = np.random.default_rng(1000 + N + M + seed)
        self.S, self.P, self.d, self.M = S, P, d, M
        X = rng.uniform(0, 1, (d, N))
        Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1] + 0.2 * np.cos(4 * X[2])])[:P]
        self.Y = Y
        lam = rng.uniform(0.35, 0.8, (P, d, S))
        amp = rng.uniform(0.8, 1.5, (P, S))
        sig = rng.uniform(0.04, 0.1, (P, S))
        c = rng.uniform(-0.2, 0.2, (S, P))
        gr = rng.uniform(-0.2, 0.2, (S, P, d))
        mean = lambda s, p, Z: c[s, p] + gr[s, p] @ Z                                     # noqa: E731
        self.mean = mean
        self.Xs = np.asfortranarray(rng.uniform(-0.05, 1.05, (d, M)))
        self.mask = O.in_bounds(self.Xs, np.zeros(d), np.ones(d))
        self.gps = [[None] * P for _ in range(S)]
        self.status = []
        for p in range(P):
            a = amp[p].copy()
            if bad_sample is not None and p == 0:
                a[bad_sample] = -1.0                                                      # fit_batch returns this member unfitted
            mX = np.stack([mean(s, p, X) for s in range(S)])
            gp, _, st = api.fit_batch(X, Y[p], kernel, lam[p], a, sig[p], mean_X=mX)
            self.status.append(st)
            for s in range(S):
                self.gps[s][p] = gp[s]
        self.posts = [[O.gp_fit(X, Y[p], kernel, lam[p][:, s], amp[p, s], sig[p, s], mean=mean(s, p, X)) for p in range(P)]
                      for s in range(S)]
        self.ms = self.ms_at(self.Xs)                                                                        # S×P×M
        self.mg = np.stack([np.stack([np.repeat(gr[s, p][:, None], M, axis=1) for p in range(P)]) for s in range(S)])   # S×P×d×M
        self.coefs = [1.0, 0.2][:P]

    def ms_at(self, Z):
        return np.stack([np.stack([self.mean(s, p, Z) for p in range(self.P)]) for s in range(self.S)])

    def args(self, O, mode):
        y_max = [np.inf, 0.3][:self.P] if mode in ("both", "cons_only") else None
        b = O.best_so_far(self.coefs, self.Y, [np.inf, 0.3][:self.P]) if mode in ("both", "best_only") else None
        return y_max, b

    def oracle(self, O, mode, samples=None):
        y_max, b = self.args(O, mode)
        samples = range(self.S) if samples is None else samples
        res = [O.ei_acquisition_grad(self.posts[s], self.Xs, self.coefs, y_max, b, valid_mask=self.mask, means_s=list(self.ms[s]),
                                     mean_grads_s=list(self.mg[s])) for s in samples]
        return sum(r[0] for r in res) / len(res), sum(r[1] for r in res) / len(res)

    def device(self, api, O, mode, samples=None):
        y_max, b = self.args(O, mode)
        samples = list(range(self.S)) if samples is None else list(samples)
        return api.acq_ei_grad_set([self.gps[s] for s in samples], self.Xs, self.coefs, y_max, b, self.mask, self.ms[samples],
                                   self.mg[samples])

    def close(self):
        for row in self.gps:
            for g in row:
                g.close()


def assert_plain(acq, dacq, acq_o, dacq_o, mask, what, factor=1.0):
    """the bounds of tests/test_gpu_parity.py:1073-1075 (factor 2: two results that each meet them, compared with each other)"""
    ea, eg = np.abs(acq - acq_o).max(), np.abs(dacq - dacq_o).max()
    print(f"{what}: |dacq| {ea:.3e} (<= {factor * 1e-11:.1e})  |dgrad| {eg:.3e} (<= {factor * 1e-9 * (1 + np.abs(dacq_o).max()):.3e})", flush=True)
    assert ea <= factor * 1e-11, (what, ea)
    assert eg <= factor * 1e-9 * (1.0 + np.abs(dacq_o).max()), (what, eg)
    assert np.all(dacq[:, ~mask] == 0.0) and np.all(acq[~mask] == 0.0), what


def run_plain(api, O, N, M, kernel):
    case = Plain(api, O, N, M, kernel)
    try:
        before = api._set_grad_launches()
        for mode in MODES:
            acq, dacq = case.device(api, O, mode)
            acq_o, dacq_o = case.oracle(O, mode)
            assert_plain(acq, dacq, acq_o, dacq_o, case.mask, f"plain N={N} M={M} {kernel} {mode}")
        assert api._set_grad_launches() > before or os.environ.get("BOSS_NO_SET_PREDICT") == "1"
    finally:
        case.close()


def grad_case(n, d, S, seed=0):
    """y = sin(Xᵀw) with its exact gradient and S parameter draws (as tests/test_gpu_model_fit_batch.py)."""
    rng = np.random.default_rng(100 + seed)
    X = rng.uniform(0, 1, (d, n))
    w = rng.uniform(0.5, 2.0, d)
    y = np.sin(X.T @ w)
    dY = w[:, None] * np.cos(X.T @ w)[None, :]
    lam = rng.uniform(0.3, 1.5, (d, S))
    amp, sig, sgd = rng.uniform(0.5, 2.0, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
    return X, y, dY, lam, amp, sig, sgd


def run_grad_model(api, O, n, M, kernel="matern52"):
    d, S = D_, S_
    X, y, dY, lam, amp, sig, sgd = grad_case(n, d, S, seed=n + M)
    Xs = np.asfortranarray(np.random.default_rng(M).uniform(0.05, 0.95, (d, M)))
    best = float(y.max()) - 0.3
    gps, _, st = api.ggp_fit_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    try:
        assert not st.any()
        acc, gacc, tol_a, tol_g = 0.0, 0.0, 0.0, 0.0
        for s in range(S):
            post = O.gradient_gp_fit(X, y, dY, kernel, lam[:, s], amp[s], sig[s], sgd[s])
            mu_o, var_o, dmu_o, dvar_o = O.gradient_gp_mean_and_var_grad(post, Xs)
            vo = np.maximum(var_o, 0.0)
            a_o, g_o = O.expected_improvement_lin_grad([1.0], mu_o[None], vo[None], dmu_o[None], np.where(vo > 0, dvar_o, 0.0)[None], best)
            K = O.augmented_kernel_matrix(kernel, X, lam[:, s], amp[s], sig[s], sgd[s])
            tol = max(1e-9, np.linalg.cond(K) * K.shape[0] * 2.0 ** -53 * 8)
            acc, gacc = acc + a_o, gacc + g_o
            tol_a += tol * 10 / S
            tol_g += tol * (1 + np.abs(g_o).max()) * 100 / S
        acq_o, dacq_o = acc / S, gacc / S
        before = api._set_grad_launches()
        acq, dacq = api.acq_ei_grad_set([[g] for g in gps], Xs, [1.0], None, best)
        assert api._set_grad_launches() > before or os.environ.get("BOSS_NO_SET_PREDICT") == "1"
        ea, eg = np.abs(acq - acq_o).max(), np.abs(dacq - dacq_o).max()
        print(f"gradient model n={n} M={M}: |dacq| {ea:.3e} (<= {tol_a:.3e})  |dgrad| {eg:.3e} (<= {tol_g:.3e})", flush=True)
        assert ea <= tol_a and eg <= tol_g, (ea, tol_a, eg, tol_g)
    finally:
        for g in gps:
            g.close()


# ------------------------------------------------------------------------------------------ 1, 2: against the oracle
@pytest.mark.parametrize("N,M,kernel", PLAIN_CASES)
def test_plain_members_against_the_oracle(api, O, N, M, kernel):
    """Members of fit_batch (S = 5, P = 2, d = 3, per-sample prior means with gradients, mask), all four construct_ei variants:
    |Δacq| <= 1e-11, |Δ∇acq| <= 1e-9 (1 + max|∇acq_oracle|), zeros under the mask (tests/test_gpu_parity.py:1073-1075)."""
    run_plain(api, O, N, M, kernel)


@pytest.mark.parametrize("n,M", GRAD_CASES)
def test_gradient_model_members_against_the_oracle(api, O, n, M):
    """Members of ggp_fit_batch, n (1 + d) = 240 and 260 rows, against the mean over s of gradient_gp_mean_and_var_grad +
    expected_improvement_lin_grad.  Tolerance of the single-member test, tests/test_gpu_parity.py:1695,1706-1707, per member
    (tol_s = max(1e-9, cond(K_s) rows 2^-53 8); |Δacq| <= 10 tol_s, |Δ∇acq| <= 100 tol_s (1 + max|∇acq_s|)), averaged over s."""
    run_grad_model(api, O, n, M)


# ------------------------------------------------------------------------------------------ 3: set against loop
def test_set_equals_the_loop_over_samples(api, O):
    """The set result against the mean of S api.acq_ei_grad calls: within twice the oracle bounds (both meet them; the two paths
    use different adjoint kernels, so no bitwise agreement)."""
    case = Plain(api, O, 260, 70, "matern52")
    try:
        for mode in MODES:
            y_max, b = case.args(O, mode)
            acq, dacq = case.device(api, O, mode)
            loop = [api.acq_ei_grad(case.gps[s], case.Xs, case.coefs, y_max, b, case.mask, case.ms[s], case.mg[s]) for s in range(case.S)]
            acq_l, dacq_l = sum(r[0] for r in loop) / case.S, sum(r[1] for r in loop) / case.S
            _, dacq_o = case.oracle(O, mode)
            ea, eg = np.abs(acq - acq_l).max(), np.abs(dacq - dacq_l).max()
            print(f"set vs loop {mode}: |dacq| {ea:.3e}  |dgrad| {eg:.3e}", flush=True)
            assert ea <= 2e-11 and eg <= 2e-9 * (1 + np.abs(dacq_o).max()), (mode, ea, eg)
    finally:
        case.close()


# ------------------------------------------------------------------------------------------ 4: path and determinism
def test_path_and_determinism(api, O):
    """Members of one fit take the set launches; the first call after the fit (which builds the transposed factors) and the second
    give bitwise identical outputs, for the plain and the gradient-observation model; S = 1 is api.acq_ei_grad bit for bit."""
    case = Plain(api, O, 260, 70, "matern52")
    try:
        before = api._set_grad_launches()
        r1 = case.device(api, O, "both")                          # first call after the fit
        assert api._set_grad_launches() > before, "members of one fit did not take the set launches"
        r2 = case.device(api, O, "both")
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]), "two consecutive calls differ (plain model)"
        y_max, b = case.args(O, "both")
        one = api.acq_ei_grad_set([case.gps[2]], case.Xs, case.coefs, y_max, b, case.mask, case.ms[2:3], case.mg[2:3])
        ref = api.acq_ei_grad(case.gps[2], case.Xs, case.coefs, y_max, b, case.mask, case.ms[2], case.mg[2])
        assert np.array_equal(one[0], ref[0]) and np.array_equal(one[1], ref[1]), "S = 1 differs from acq_ei_grad"
    finally:
        case.close()
    X, y, dY, lam, amp, sig, sgd = grad_case(65, D_, S_, seed=7)
    Xs = np.asfortranarray(np.random.default_rng(7).uniform(0.05, 0.95, (D_, 70)))
    gps, _, st = api.ggp_fit_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
    try:
        assert not st.any()
        best = float(y.max()) - 0.3
        before = api._set_grad_launches()
        r1 = api.acq_ei_grad_set([[g] for g in gps], Xs, [1.0], None, best)   # first call after the fit
        assert api._set_grad_launches() > before
        r2 = api.acq_ei_grad_set([[g] for g in gps], Xs, [1.0], None, best)
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]), "two consecutive calls differ (gradient model)"
        one = api.acq_ei_grad_set([[gps[3]]], Xs, [1.0], None, best)
        ref = api.acq_ei_grad([gps[3]], Xs, [1.0], None, best)
        assert np.array_equal(one[0], ref[0]) and np.array_equal(one[1], ref[1])
    finally:
        for g in gps:
            g.close()


def test_repeat_is_bitwise_without_row_split(api, O):
    """64 samples × 2 outputs at 224 candidates: 7 tiles × 128 members = 896 workgroups, so the accumulation runs without the row
    split (the cases above take it); first call after the fit against the second, bit for bit."""
    case = Plain(api, O, 260, 224, "matern52", S=64)
    try:
        before = api._set_grad_launches()
        r1 = case.device(api, O, "both")
        assert api._set_grad_launches() > before
        r2 = case.device(api, O, "both")
        assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
        acq_o, dacq_o = case.oracle(O, "both")
        assert_plain(r1[0], r1[1], acq_o, dacq_o, case.mask, "plain S=64 N=260 M=224")
    finally:
        case.close()


def run_mixed(api, O):
    """samples 0-2 on N = 260 points, samples 3-4 on N = 300: no common shape, so no set launch; same bounds.  Returns whether
    the set-launch counter rose."""
    a, b = Plain(api, O, 260, 70, "matern52", S=3, seed=1), Plain(api, O, 300, 70, "matern52", S=2, seed=2)
    try:
        y_max, bb = a.args(O, "both")
        ms_b = b.ms_at(a.Xs)                                      # b's prior means at the shared candidates
        before = api._set_grad_launches()
        acq, dacq = api.acq_ei_grad_set(a.gps + b.gps, a.Xs, a.coefs, y_max, bb, a.mask, np.concatenate([a.ms, ms_b]),
                                        np.concatenate([a.mg, b.mg]))
        rose = api._set_grad_launches() > before
        res = [O.ei_acquisition_grad(c.posts[s], a.Xs, a.coefs, y_max, bb, valid_mask=a.mask, means_s=list(m[s]), mean_grads_s=list(c.mg[s]))
               for c, m in ((a, a.ms), (b, ms_b)) for s in range(c.S)]
        acq_o, dacq_o = sum(r[0] for r in res) / len(res), sum(r[1] for r in res) / len(res)
        assert_plain(acq, dacq, acq_o, dacq_o, a.mask, "mixed N")
        return rose
    finally:
        a.close(), b.close()


def test_mixed_shapes_go_member_by_member(api, O):
    assert not run_mixed(api, O), "a list mixing two N took the set launches"


CHILD_NO_SET = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
entry.build()
from boss_jl_amd import api
from oracle import gp_oracle as O
import test_gpu_acq_grad_set as T
before = api._set_grad_launches()
T.run_plain(api, O, 260, 70, "matern52")
T.run_grad_model(api, O, 65, 70)
assert api._set_grad_launches() == before, "BOSS_NO_SET_PREDICT=1 still took the set launches"
print("RES ok")
'''


def test_switch_turns_the_set_launches_off(api):
    """BOSS_NO_SET_PREDICT=1 (read once: a child process): member by member inside the call, same bounds."""
    code = CHILD_NO_SET % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BOSS_NO_SET_PREDICT="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RES ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------ 5: errors
def test_errors_leave_the_handles_usable(api, O):
    case = Plain(api, O, 260, 70, "matern52", bad_sample=1)
    rng = np.random.default_rng(3)
    ns = api.GibbsGP(rng.uniform(0, 1, (D_, 50)), rng.standard_normal(50))
    X2 = rng.uniform(0, 1, (2, 260))
    g2 = api.GP(X2, np.sin(3 * X2).sum(0), "matern52")
    g2.update([0.5, 0.5], 1.0, 0.05)
    try:
        assert case.status[0][1] == api.BOSS_E_INVALID and not case.status[1].any()
        y_max, b = case.args(O, "both")
        good = [0, 2, 3, 4]

        def call(rows, ms, mg):
            return api.acq_ei_grad_set(rows, case.Xs, case.coefs, y_max, b, case.mask, ms, mg)

        def good_call(what):
            acq, dacq = call([case.gps[s] for s in good], case.ms[good], case.mg[good])
            acq_o, dacq_o = case.oracle(O, "both", good)
            assert_plain(acq, dacq, acq_o, dacq_o, case.mask, what)

        with pytest.raises(api.BossError) as e:
            call(case.gps, case.ms, case.mg)                      # sample 1, output 0 came back unfitted
        assert e.value.code == api.BOSS_E_NOT_FITTED
        good_call("after NOT_FITTED")
        with pytest.raises(api.BossError) as e:
            call([case.gps[0], [ns, case.gps[2][1]]], case.ms[[0, 2]], case.mg[[0, 2]])
        assert e.value.code == api.BOSS_E_INVALID
        good_call("after a nonstationary handle")
        with pytest.raises(api.BossError) as e:
            call([case.gps[0], [g2, case.gps[2][1]]], case.ms[[0, 2]], case.mg[[0, 2]])
        assert e.value.code == api.BOSS_E_INVALID
        good_call("after mismatched x_dim")
    finally:
        case.close(), ns.close(), g2.close()


# ------------------------------------------------------------------------------------------ 6: poisoned allocations
CHILD_POISON = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
entry.build()
from boss_jl_amd import api
from oracle import gp_oracle as O
import test_gpu_acq_grad_set as T
for N, M, kernel in T.PLAIN_CASES:
    T.run_plain(api, O, N, M, kernel)
for n, M in T.GRAD_CASES:
    T.run_grad_model(api, O, n, M)
print("RES ok")
'''


def test_poisoned_allocations(api):
    """Tests 1 and 2 once more with every fresh device block filled with NaN patterns (BOSS_POISON_ALLOC=1, a child process):
    nothing passes on memory the set kernels never wrote."""
    code = CHILD_POISON % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BOSS_POISON_ALLOC="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RES ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------ 7: the maximiser
def test_maximizer_on_bi_samples(api, O):
    """HipGradientAM on a BI problem (S = 8, N = 300, d = 2, 64 starts, 10 iterations): the point is in the domain and its averaged
    acquisition, recomputed by the oracle, is at least the oracle acquisition of the best start."""
    import boss_jl_amd as B
    rng = np.random.default_rng(4)
    d, N, S = 2, 300, 8
    X = rng.uniform(0, 1, (d, N))
    Y = (np.sin(5 * X[0]) * np.cos(3 * X[1]) + 0.5 * X[0] + 0.05 * rng.standard_normal(N))[None, :]
    prms = [B.HipGPParams(rng.uniform(0.2, 0.4, (d, 1)), [rng.uniform(0.8, 1.3)], [rng.uniform(0.04, 0.08)]) for _ in range(S)]
    model = B.HipGaussianProcess([None], [None], [None])
    prob = B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0])), model,
                         B.ExperimentData(X, Y), None, prms)
    am = B.HipGradientAM(x_prior=lambda r: r.uniform(0, 1, d), multistart=64, iters=10, seed=2)
    before = api._set_grad_launches()
    x, val = am.maximize_acquisition(prob)
    assert api._set_grad_launches() > before, "the BI maximiser did not take the set call"
    assert x.shape == (d,) and np.all(x >= 0) and np.all(x <= 1)
    posts = [O.gp_fit(X, Y[0], "matern52", p.lengthscales[:, 0], float(np.asarray(p.amplitudes)[0]), float(np.asarray(p.noise_std)[0]))
             for p in prms]
    b = float(Y.max())
    avg = lambda Z: sum(O.ei_acquisition([post], Z, [1.0], [np.inf], b) for post in posts) / S   # noqa: E731
    a_x = avg(x[:, None])[0]
    assert abs(a_x - val) <= 1e-10, (a_x, val)
    starts_rng = np.random.default_rng(2)
    S0 = np.stack([starts_rng.uniform(0, 1, d) for _ in range(64)], axis=1)
    assert a_x >= avg(S0).max() - 1e-12, (a_x, avg(S0).max())
