"""GPU tests (pytest -m gpu) of the likelihood gradient through the prior mean: boss_gp_loglike_grad_batch_mean and
boss_gp_loglike_grad_mean on the three gradient paths (one workgroup per set for N <= 128, grouped passes up to 2048 padded rows,
set after set over the stream banks above), the model layer and the gradient fitters over a Semiparametric model.

Reference: a = K⁻¹(y − m) and dθ = Jᵀa by numpy.linalg.solve on the oracle's kernelmatrix plus noise.  Bound: the project's own
(tests/test_gpu_model_llgrad_batch.py) —
    tol = max(1e-9, cond(K)·N·2⁻⁵³·8),   error <= 100·tol·(1 + max|want|),
with noise_std >= 0.05, so that the bar stays far below the values.  Everything else is compared bit for bit.

Run as a script (`python tests/test_gpu_semipar_llgrad.py <path> <out.npz>`) the module evaluates one path's batch in a fresh
process: the chunk test starts it with BOSS_MODEL_BATCH_CHUNK_MB set (the library reads it once per process).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


def grad_tol(cond, rows):
    return max(1e-9, cond * rows * 2.0 ** -53 * 8)


# path -> (N, d, S, T, kernel): the smallest shapes that reach each kernel
PATHS = {
    "small20": (20, 2, 4, 3, "matern52"),                        # one workgroup per set (small_llgrad_kernel)
    "small128": (128, 8, 4, 1, "sqexp"),                         # ... at its largest size, two rows per lane, one column
    "group200": (200, 3, 5, 3, "matern32"),                      # Np = 256: grouped passes, grid.z = set (mean_fold_kernel)
    "group300": (300, 2, 4, 3, "matern52"),                      # Np = 512: 212 padded rows that must never be read into a result
    "set2100": (2100, 2, 5, 3, "matern52"),                      # Np = 2304: set after set, the fifth set reuses bank 0
}


@functools.lru_cache(maxsize=None)
def case(path, dup=False):
    """Data, S parameter sets (λ ∈ [0.3, 0.9], α ∈ [0.7, 1.4], σ ∈ [0.05, 0.15]), per-set means and per-set Jacobians."""
    N, d, S, T, kernel = PATHS[path]
    rng = np.random.default_rng(N + 7 * T)
    X = rng.uniform(0, 1, (d, N))
    if dup:
        X[:] = X[:, :1]                                         # identical points: with zero noise not positive definite
    y = np.sin(3 * X).sum(0) / np.sqrt(d) + 0.1 * rng.standard_normal(N)
    lam = rng.uniform(0.3, 0.9, (d, S)) * np.sqrt(d)
    amp, sig = rng.uniform(0.7, 1.4, S), rng.uniform(0.05, 0.15, S)
    means = np.stack([0.1 * X[0] + 0.05 * k * np.cos(2 * X[-1]) for k in range(S)])
    J = rng.standard_normal((S, N, T))
    return X, y, lam, amp, sig, means, J, kernel


@functools.lru_cache(maxsize=None)
def reference(path):
    """Per set: (a, Jᵀa, cond(K)) — computed once and shared."""
    from oracle import gp_oracle as O
    X, y, lam, amp, sig, means, J, kernel = case(path)
    out = []
    for s in range(lam.shape[1]):
        h = O.finite_gp_params(kernel, X.shape[0], lam[:, s], amp[s], sig[s])
        K = O.kernelmatrix(h, X)
        K[np.diag_indices(X.shape[1])] += h.noise_std ** 2
        a = np.linalg.solve(K, y - means[s])
        ev = np.linalg.eigvalsh(K)                               # (symmetric positive definite: cond = λmax / λmin)
        out.append((a, J[s].T @ a, float(ev[-1] / ev[0])))
    return out


@functools.lru_cache(maxsize=None)
def batch(path):
    """The whole batch in one call, per-set means and per-set Jacobians: (ll, st, grad, dmean, dtheta)."""
    from boss_jl_amd import api
    X, y, lam, amp, sig, means, J, kernel = case(path)
    return api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, means, J, want_dmean=True)


def same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("path", list(PATHS))
def test_dmean_and_dtheta_match_the_reference(api, path):
    N, d, S, T, _ = PATHS[path]
    ll, st, gr, dm, dth = batch(path)
    assert not st.any() and dm.shape == (N, S) and dth.shape == (T, S)
    for s, (a, dt, cond) in enumerate(reference(path)):
        tol = grad_tol(cond, N)
        for name, got, want in (("dmean", dm[:, s], a), ("dtheta", dth[:, s], dt)):
            err, bar = np.abs(got - want).max(), 100 * tol * (1 + np.abs(want).max())
            print(f"[semipar-llgrad] {path} set {s} {name}: max|d| {err:.3e} (bar {bar:.3e}, max|want| {np.abs(want).max():.3e}) cond {cond:.3e}")
            assert err <= bar, (path, s, name, err, bar)


# ------------------------------------------------------------------------------------------ 2.-5. bit for bit
@pytest.mark.parametrize("path", list(PATHS))
def test_shared_jacobian_equals_the_repeated_one(api, path):
    X, y, lam, amp, sig, means, J, kernel = case(path)
    S = lam.shape[1]
    shared = api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, means, J[1], want_dmean=True)               # jac_stride = 0
    repeated = api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, means, np.stack([J[1]] * S), want_dmean=True)
    assert same(shared, repeated)
    assert np.array_equal(shared[4][:, 1], batch(path)[4][:, 1])                                                  # set 1 had that matrix before
    # the mean values may be absent while the Jacobian is given; no fold without a Jacobian
    free = api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, None, J[1], want_dmean=True)
    plain = api.loglike_batch(X, y, kernel, lam, amp, sig, None, want_grad=True)
    assert same(free[:3], plain) and np.isfinite(free[4]).all() and free[4].any()
    none = api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, means, None, want_dmean=True)
    assert none[4] is None and np.array_equal(none[3], batch(path)[3])


@pytest.mark.parametrize("path", list(PATHS))
def test_likelihoods_and_gradients_are_those_of_the_gradient_batch(api, path):
    X, y, lam, amp, sig, means, J, kernel = case(path)
    assert same(batch(path)[:3], api.loglike_batch(X, y, kernel, lam, amp, sig, means, want_grad=True))


@pytest.mark.parametrize("path", list(PATHS))
def test_every_set_alone_equals_its_column_and_calls_repeat(api, path):
    X, y, lam, amp, sig, means, J, kernel = case(path)
    whole = batch(path)
    for s in range(lam.shape[1]):
        one = api.loglike_grad_batch_mean(X, y, kernel, lam[:, s:s + 1], amp[s:s + 1], sig[s:s + 1], means[s:s + 1], J[s:s + 1],
                                          want_dmean=True)
        assert one[0][0] == whole[0][s] and one[1][0] == whole[1][s], (path, s)
        assert all(np.array_equal(one[k][:, 0], whole[k][:, s]) for k in (2, 3, 4)), (path, s)
    again = api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, means, J, want_dmean=True)
    assert same(again, whole)


# ------------------------------------------------------------------------------------------ 6. local failures
@pytest.mark.parametrize("path", list(PATHS))
def test_failed_sets_get_zero_columns_and_leave_their_neighbours_alone(api, path):
    """Identical points with zero noise are not positive definite (tests/test_gpu_model_llgrad_batch.py), a negative lengthscale
    is invalid; the good sets of that data (K = α²·11ᵀ + σ²I) are compared with a batch of their own."""
    X, y, lam, amp, sig, means, J, kernel = case(path, dup=True)
    S = lam.shape[1]
    good = [s for s in range(S) if s not in (1, 2)]
    lam, sig = lam.copy(), sig.copy()
    sig[1] = 0.0                                                 # not PD
    lam[0, 2] = -0.1                                             # invalid
    ll, st, gr, dm, dth = api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, means, J, want_dmean=True)
    assert st[1] == api.BOSS_E_NOT_PD and st[2] == api.BOSS_E_INVALID and ll[1] == ll[2] == -np.inf
    for bad in (1, 2):
        assert not gr[:, bad].any() and not dm[:, bad].any() and not dth[:, bad].any()
    ref = api.loglike_grad_batch_mean(X, y, kernel, lam[:, good], amp[good], sig[good], means[good], J[good], want_dmean=True)
    assert not ref[1].any() and not st[good].any()
    assert np.array_equal(ll[good], ref[0]) and all(np.array_equal(a[:, good], b) for a, b in zip((gr, dm, dth), ref[2:]))


def test_argument_checks(api):
    X, y, lam, amp, sig, means, J, kernel = case("small20")
    N, d, S, T, _ = PATHS["small20"]
    lib = api.load_library()
    import ctypes as C
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
    Xf, lamf = np.asfortranarray(X), np.asfortranarray(lam)
    Jf = np.ascontiguousarray(J.transpose(0, 2, 1))
    ll, gr, dm, dth, st = np.zeros(S), np.zeros((d + 2) * S), np.zeros(N * S), np.zeros(T * S), np.zeros(S, dtype=np.int32)

    def call(T_, jac, stride, dth_, S_=S):
        return lib.boss_gp_loglike_grad_batch_mean(0, api.KERNELS[kernel], d, N, dp(Xf), dp(y), None, 0, None, S_, dp(lamf), dp(amp), dp(sig),
                                                   T_, dp(jac), stride, dp(ll), dp(gr), dp(dm), dp(dth_), st.ctypes.data_as(C.POINTER(C.c_int)))
    assert call(-1, Jf, 0, None) == api.BOSS_E_INVALID
    assert call(T, None, 0, dth) == api.BOSS_E_INVALID
    assert call(T, Jf, N * T + 1, dth) == api.BOSS_E_INVALID and call(T, Jf, N, dth) == api.BOSS_E_INVALID
    assert call(0, None, 0, dth) == api.BOSS_E_INVALID
    assert call(T, Jf, N * T, dth, S_=0) == api.BOSS_OK and not dth.any()                  # S = 0: nothing happens
    assert call(T, Jf, N * T, dth) == api.BOSS_OK and np.array_equal(dth.reshape(T, S, order="F"), batch_nomean("small20"))


@functools.lru_cache(maxsize=None)
def batch_nomean(path):
    from boss_jl_amd import api
    X, y, lam, amp, sig, means, J, kernel = case(path)
    return api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, None, J)[4]


# ------------------------------------------------------------------------------------------ 7. chunks
def test_three_chunks_agree_bitwise_with_one(api, tmp_path):
    """N = 200: a set's matrix takes (256 + 128)·256·8 bytes = 0.75 MiB, so BOSS_MODEL_BATCH_CHUNK_MB=1.6 (read once per process,
    hence a child) holds two sets per chunk and the five sets span three chunks."""
    out = os.path.join(str(tmp_path), "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "group200", out], env=dict(os.environ, BOSS_MODEL_BATCH_CHUNK_MB="1.6"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = np.load(out)
    whole = batch("group200")
    assert all(np.array_equal(got[k], whole[i]) for i, k in enumerate(("ll", "st", "gr", "dm", "dth")))


# ------------------------------------------------------------------------------------------ single handle
@pytest.mark.parametrize("path", ["small20", "group300"])
def test_single_handle(api, path):
    X, y, lam, amp, sig, means, J, kernel = case(path)
    N = X.shape[1]
    a, _, cond = reference(path)[0]
    g = api.GP(X, y, kernel)
    lp = g.update(lam[:, 0], amp[0], sig[0], means[0])
    lp1, gr1 = g.loglike_grad()
    lp2, gr2, dm = g.loglike_grad_mean()
    assert lp2 == lp1 == lp and np.array_equal(gr1, gr2) and dm.shape == (N,)
    err, bar = np.abs(dm - a).max(), 100 * grad_tol(cond, N) * (1 + np.abs(a).max())
    print(f"[semipar-llgrad] handle {path}: max|d dmean| {err:.3e} (bar {bar:.3e}) cond {cond:.3e}")
    assert err <= bar
    lp3, gr3, dm3 = g.loglike_grad_mean()                         # repeatable, and the handle still serves the old call
    assert lp3 == lp2 and np.array_equal(gr3, gr2) and np.array_equal(dm3, dm) and np.array_equal(g.loglike_grad()[1], gr1)
    g.close()


def test_single_handle_after_an_append_across_the_small_limit(api, O):
    """127 points (one workgroup) + 2 appended = 129 (the general path): dmean has the handle's current count and matches a fresh
    fit's to the reference's bound."""
    rng = np.random.default_rng(5)
    d, N = 3, 129
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(3 * X).sum(0) + 0.1 * rng.standard_normal(N)
    mean = 0.2 * X[1]
    lam, amp, sig = np.array([0.5, 0.6, 0.7]), 1.1, 0.08
    g = api.GP(X[:, :127], y[:127], "matern52")
    g.reserve(N)
    g.update(lam, amp, sig, mean[:127])
    assert g.loglike_grad_mean()[2].shape == (127,)
    g.append(X[:, 127:], y[127:], mean[127:])
    lp, gr, dm = g.loglike_grad_mean()
    f = api.GP(X, y, "matern52")
    f.update(lam, amp, sig, mean)
    lpf, grf, dmf = f.loglike_grad_mean()
    h = O.finite_gp_params("matern52", d, lam, amp, sig)
    K = O.kernelmatrix(h, X)
    K[np.diag_indices(N)] += h.noise_std ** 2
    a = np.linalg.solve(K, y - mean)
    tol = grad_tol(np.linalg.cond(K), N)
    assert dm.shape == dmf.shape == (N,)
    for name, got in (("appended", dm), ("fresh", dmf)):
        err, bar = np.abs(got - a).max(), 100 * tol * (1 + np.abs(a).max())
        print(f"[semipar-llgrad] {name} handle: max|d dmean| {err:.3e} (bar {bar:.3e})")
        assert err <= bar
    assert abs(lp - lpf) <= tol * (1 + abs(lpf)) and np.abs(gr - grf).max() <= 100 * tol * (1 + np.abs(grf).max())
    g.close()
    f.close()


def test_other_models_handles_are_refused_and_stay_usable(api):
    rng = np.random.default_rng(6)
    d, n = 2, 12
    X, y, dY = rng.uniform(0, 1, (d, n)), rng.standard_normal(n), rng.standard_normal((d, n))
    gg = api.GradGP(X, y, dY, "sqexp")
    gg.update([0.5, 0.6], 1.0, 0.1, 0.1)
    before = gg.loglike_grad()
    with pytest.raises(api.BossError) as e:
        gg.loglike_grad_mean()
    assert e.value.code == api.BOSS_E_INVALID
    after = gg.loglike_grad()
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    gg.close()
    ng = api.GibbsGP(X, y)
    ng.update(np.full((d, n), 0.5), np.ones(n), np.full(n, 0.1))
    before = ng.loglike_grad()
    with pytest.raises(api.BossError) as e:
        ng.loglike_grad_mean()
    assert e.value.code == api.BOSS_E_INVALID
    after = ng.loglike_grad()
    assert before[0] == after[0] and all(np.array_equal(p, q) for p, q in zip(before[1:], after[1:]))
    ng.close()
    fresh = api.GP(X, y, "sqexp")                                # not fitted yet
    with pytest.raises(api.BossError):
        fresh.loglike_grad_mean()
    fresh.close()


# ------------------------------------------------------------------------------------------ model layer and fitters
def _mean(x, th):
    return np.array([th[0] + th[1] * x[0] + np.cos(th[2] * x[1]), 0.5 * th[0] - th[1] * x[1] + np.cos(th[2] * x[0])])


def _mean_jac(x, th):
    return np.array([[1.0, x[0], -x[1] * np.sin(th[2] * x[1])], [0.5, -x[1], -x[0] * np.sin(th[2] * x[0])]])


TRUTH = np.array([0.8, -0.6, 1.3])


@functools.lru_cache(maxsize=None)
def semipar_problem(noise=0.02):
    """P = 2, N = 24, d = 2: an affine-plus-cosine mean with T = 3 at TRUTH plus a small smooth term and noise."""
    import boss_jl_amd as B
    rng = np.random.default_rng(8)
    d, N, P = 2, 24, 2
    X = rng.uniform(0, 2, (d, N))
    Y = np.stack([[_mean(X[:, j], TRUTH)[i] for j in range(N)] for i in range(P)]) + noise * rng.standard_normal((P, N))
    model = B.HipGaussianProcess(lengthscale_priors=[B.MvLogNormal([-0.5, -0.5], [0.3, 0.3])] * P, amplitude_priors=[B.LogNormal(-2.5, 0.3)] * P,
                                 noise_std_priors=[B.LogNormal(-3.5, 0.3)] * P, parametric=_mean, parametric_jac=_mean_jac,
                                 theta_priors=[B.Normal(0.0, 2.0), B.Normal(0.0, 2.0), B.Normal(1.0, 1.0)])
    return B.BossProblem(None, B.Domain((np.zeros(d), 2 * np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])), model,
                         B.ExperimentData(X, Y))


def test_theta_gradient_matches_central_differences_of_the_device_likelihood(api):
    """∂/∂θ of data_loglike_grad_batch against central differences (eps 1e-5) of the device's own data_loglike_batch values, with
    the bound of tests/test_gpu_parity.py's finite-difference check of boss_gp_loglike_grad: |got − want| <= 2e-5 (1 + |want|)."""
    import boss_jl_amd as B
    prob = semipar_problem()
    model, data = prob.model, prob.data
    rng = np.random.default_rng(9)
    sampler = model.params_sampler()
    plist = [sampler(rng) for _ in range(3)]
    ll, grads = model.data_loglike_grad_batch(data, plist)
    assert np.array_equal(ll, model.data_loglike_batch(data, plist))
    eps = 1e-5
    for k, p in enumerate(plist):
        for t in range(3):
            up, dn = p.theta.copy(), p.theta.copy()
            up[t] += eps
            dn[t] -= eps
            f = model.data_loglike_batch(data, [B.HipGPParams(p.lengthscales, p.amplitudes, p.noise_std, up),
                                                B.HipGPParams(p.lengthscales, p.amplitudes, p.noise_std, dn)])
            want, got = (f[0] - f[1]) / (2 * eps), grads[k].theta[t]
            print(f"[semipar-llgrad] start {k} theta {t}: got {got:.9e} central differences {want:.9e}")
            assert abs(got - want) <= 2e-5 * (1 + abs(want)), (k, t, got, want)
    # the numeric Jacobian gives the same gradient up to its own error (model.py: about 1e-9 of the mean's size, times Σ|a|)
    numeric = B.HipGaussianProcess(model.lengthscale_priors, model.amplitude_priors, model.noise_std_priors, parametric=_mean,
                                   theta_priors=model.theta_priors)
    _, g2 = numeric.data_loglike_grad_batch(data, plist)
    for a, b in zip(grads, g2):
        assert np.abs(a.theta - b.theta).max() <= 1e-6 * (1 + np.abs(a.theta).max())


def test_gradient_map_climbs_and_moves_theta(api):
    import boss_jl_amd as B
    prob = semipar_problem()
    start = B.HipGradientMAP(multistart=4, iters=0, seed=3).estimate_parameters(prob, return_all=True)
    end = B.HipGradientMAP(multistart=4, iters=30, seed=3).estimate_parameters(prob, return_all=True)
    assert len(end) == 4
    for s, e in zip(start, end):
        assert np.isfinite(s.loglike) and e.loglike >= s.loglike and not np.array_equal(e.params.theta, s.params.theta)
    # data generated from TRUTH with small noise: the fit ends closer to it than its best start
    best_start = max(start, key=lambda r: r.loglike)
    best = B.HipGradientMAP(multistart=4, iters=30, seed=3).estimate_parameters(prob)
    d0, d1 = np.linalg.norm(best_start.params.theta - TRUTH), np.linalg.norm(best.params.theta - TRUTH)
    print(f"[semipar-llgrad] |theta - truth|: best start {d0:.4f} -> fit {d1:.4f}; log-posterior {best_start.loglike:.3f} -> {best.loglike:.3f}")
    assert best.loglike == max(e.loglike for e in end) and d1 < d0


def test_sample_opt_map_runs_on_the_semiparametric_problem(api):
    import boss_jl_amd as B
    prob = semipar_problem()
    res = B.HipSampleOptMAP(samples=40, multistart=3, iters=10, seed=4).estimate_parameters(prob, return_all=True)
    assert len(res) == 3 and all(np.isfinite(r.loglike) and r.params.theta.shape == (3,) for r in res)
    scored = B.HipBatchedMAP(40, 4).estimate_parameters(prob, return_all=True)
    assert max(r.loglike for r in res) >= max(s.loglike for s in scored)


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    ll, st, gr, dm, dth = batch(sys.argv[1])
    np.savez(sys.argv[2], ll=ll, st=st, gr=gr, dm=dm, dth=dth)
