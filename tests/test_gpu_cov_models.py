"""Posterior covariance of the gradient-observation and nonstationary models on the device (boss_ggp_predict_cov,
boss_ngp_predict_cov; cov_syrk_partial_kernel + cov_finish_kernel) against Σ built from the oracle's primitives:
    gradient observations  Σ = (α+ε)² κ(‖(x_i − x_j) ⊘ (λ+ε)‖) − VᵀV,  V = L⁻¹ k*           (gradient_gp.jl:368-373)
    nonstationary          Σ = K**_Gibbs − VᵀV + 1e-18·I, diagonal through _clip_var     (gaussian_process.jl:163-167,180-184)
Tolerances are the condition-aware ones of tests/test_gpu_parity.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-8


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


def make(d, N, M, seed=1, noise=0.05, scale=1.0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, scale, (d, N))
    y = np.sin(2 * np.pi * X / scale).sum(0) / np.sqrt(d) + noise * rng.standard_normal(N)
    Xs = np.random.default_rng(seed + 1000).uniform(0, scale, (d, M))
    return X, y, Xs


def make_grad(d, n, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, n))
    w = np.linspace(1.0, 2.0, d)[:, None]
    y = np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(d)
    dY = 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(d)
    return X, y, dY


def latent(d):
    f_lam = lambda x: 0.25 + 0.5 * np.asarray(x) ** 2 + 0.1 * np.arange(1, d + 1)        # noqa: E731
    f_amp = lambda x: 1.0 + 0.4 * np.sin(3 * x[0])                                        # noqa: E731
    f_noise = lambda x: 0.03 + 0.05 * x[-1] ** 2                                           # noqa: E731
    return f_lam, f_amp, f_noise


def ev(f, Z):
    return np.array([f(Z[:, j]) for j in range(Z.shape[1])])


def grad_expected(O, post, kernel, Xs):
    """(μ, Σ, tol) of the gradient-observation slice from the oracle's primitives."""
    Ks = O.augmented_cross_cov(kernel, post.X, post.lengthscale, post.amplitude, Xs)
    V = sla.solve_triangular(post.L, Ks, lower=True, check_finite=False)
    kid = O.KERNEL_NAMES[kernel]
    Kss = (post.amplitude + EPS) ** 2 * O.kappa(kid, O.scaled_distance(Xs, Xs, post.lengthscale + EPS))
    K = post.L @ post.L.T
    tol = max(1e-9, np.linalg.cond(K) * K.shape[0] * 2.0 ** -53 * 8)
    return Ks.T @ post.alpha, Kss - V.T @ V, tol


def gibbs_expected(O, post, Xs, lamS, ampS, mS=None, disc=None):
    """(μ, unclipped Σ, tol) of the nonstationary slice from the oracle's primitives."""
    Xsr = O.discrete_round(Xs, disc)
    Ks = O.gibbs_kernel_matrix(O.discrete_round(post.X, disc), post.lam_X, post.amp_X, Xsr, lamS, ampS)
    V = sla.solve_triangular(post.L, Ks, lower=True, check_finite=False)
    S = O.gibbs_kernel_matrix(Xsr, lamS, ampS, Xsr, lamS, ampS) - V.T @ V + 1e-18 * np.eye(Xs.shape[1])
    mu, _ = O.nonstationary_mean_and_var(post, Xs, lamS, ampS, mean_s=mS, clip=False)
    K = post.L @ post.L.T
    tol = max(1e-9, np.linalg.cond(K) * K.shape[0] * 2.0 ** -53 * 8)
    return mu, S, tol


def clip_diag(O, S):
    S = S.copy()
    S[np.diag_indices(S.shape[0])] = O.clip_var(np.diag(S))
    return S


def grad_case(api, O, kernel, d, n, M, seed=5):
    X, y, dY = make_grad(d, n)
    Xs = np.asfortranarray(np.random.default_rng(seed).uniform(0, 1, (d, M)))
    Xs[:, 0] = X[:, min(2, n - 1)]                           # a candidate on a training point
    if M >= 3:
        Xs[:, 2] = Xs[:, 1]                                  # two identical candidate columns
    lam, amp = np.linspace(0.35, 0.6, d), 1.2
    post = O.gradient_gp_fit(X, y, dY, kernel, lam, amp, 0.05, 0.1)
    g = api.GradGP(X, y, dY, kernel)
    g.update(lam, amp, 0.05, 0.1)
    return X, Xs, post, g, amp


@pytest.mark.parametrize("kernel", ["matern32", "matern52", "sqexp"])
@pytest.mark.parametrize("d,n,M", [(1, 1, 3), (3, 40, 70), (8, 150, 40), (16, 70, 33), (4, 300, 1100)])
def test_gradient_gp_cov_parity(api, O, kernel, d, n, M):
    """The fused kernel (n(1+d) < 1024) and the few-candidates steps (above) leave V for the covariance kernels."""
    X, Xs, post, g, amp = grad_case(api, O, kernel, d, n, M)
    mu_o, S_o, tol = grad_expected(O, post, kernel, Xs)
    mu, S = g.predict_value_cov(Xs)
    assert S.shape == (M, M) and np.isfinite(S).all()
    assert np.array_equal(S, S.T)                            # bitwise symmetric
    assert np.abs(S - S_o).max() <= tol * amp ** 2, np.abs(S - S_o).max()
    assert np.abs(mu - mu_o).max() <= tol * (1 + np.abs(mu_o).max())
    mu_p, var_p = g.predict(Xs)
    assert np.abs(mu - mu_p).max() <= tol * (1 + np.abs(mu_p).max())
    pos = var_p > 0
    assert np.abs(np.diag(S)[pos] - var_p[pos]).max(initial=0.0) <= tol * amp ** 2
    assert np.diag(S)[~pos].min(initial=0.0) >= -tol * amp ** 2                 # rounding level where var clips to 0
    if M >= 3:
        assert np.abs(S[1] - S[2]).max() <= 1e-12 * amp ** 2 and np.abs(S[:, 1] - S[:, 2]).max() <= 1e-12 * amp ** 2
    g.close()


def test_gradient_gp_cov_repeated_calls(api, O):
    """Np = 1350 >= 1024: the first call on a fresh handle takes the few-candidates steps, the later ones the resident-inverse GEMM
    (only covariance calls in between: both kinds of call count towards the switch)."""
    kernel = "matern52"
    X, Xs, post, g, amp = grad_case(api, O, kernel, 8, 150, 40)
    mu_o, S_o, tol = grad_expected(O, post, kernel, Xs)
    res = [g.predict_value_cov(Xs) for _ in range(3)]
    for mu, S in res:
        assert np.abs(S - S_o).max() <= tol * amp ** 2 and np.abs(mu - mu_o).max() <= tol * (1 + np.abs(mu_o).max())
        assert np.array_equal(S, S.T)
    assert np.array_equal(res[1][0], res[2][0]) and np.array_equal(res[1][1], res[2][1])
    g.close()


def test_gradient_gp_cov_many_and_one_candidate(api, O):
    """M = 4200 > 4096 leaves the few-candidates path for the one-launch kernel: the full Σ restricted to a subset equals the
    covariance of a separate call on that subset, which is checked against the oracle; M = 1 as well."""
    kernel = "matern32"
    d, n, M = 7, 130, 4200
    X, y, dY = make_grad(d, n)
    Xs = np.asfortranarray(np.random.default_rng(9).uniform(0, 1, (d, M)))
    lam, amp = np.linspace(0.35, 0.6, d), 1.1
    post = O.gradient_gp_fit(X, y, dY, kernel, lam, amp, 0.05, 0.1)
    g = api.GradGP(X, y, dY, kernel)
    g.update(lam, amp, 0.05, 0.1)
    mu, S = g.predict_value_cov(Xs)
    assert S.shape == (M, M) and np.array_equal(S, S.T) and np.isfinite(S).all()
    idx = np.sort(np.random.default_rng(1).choice(M, 40, replace=False))
    idx[-1] = M - 1                                          # the last (partial) candidate tile
    Xi = np.asfortranarray(Xs[:, idx])
    mu_i, S_i = g.predict_value_cov(Xi)
    mu_o, S_o, tol = grad_expected(O, post, kernel, Xi)
    assert np.abs(S_i - S_o).max() <= tol * amp ** 2 and np.abs(mu_i - mu_o).max() <= tol * (1 + np.abs(mu_o).max())
    assert np.abs(S[np.ix_(idx, idx)] - S_i).max() <= tol * amp ** 2 and np.abs(mu[idx] - mu_i).max() <= tol * (1 + np.abs(mu_i).max())
    mu1, S1 = g.predict_value_cov(Xs[:, :1])
    mu_o1, S_o1, _ = grad_expected(O, post, kernel, Xs[:, :1])
    assert S1.shape == (1, 1) and abs(S1[0, 0] - S_o1[0, 0]) <= tol * amp ** 2 and abs(mu1[0] - mu_o1[0]) <= tol * (1 + abs(mu_o1[0]))
    g.close()


def gibbs_case(api, d, N, M, seed=4, disc=None):
    X, y, Xs = make(d, N, M, seed=seed)
    f_lam, f_amp, f_noise = latent(d)
    Xr = X.copy() if disc is None else np.where(np.asarray(disc)[:, None], np.rint(X), X)
    Xsr = Xs.copy() if disc is None else np.where(np.asarray(disc)[:, None], np.rint(Xs), Xs)
    lamX, ampX, noiX = ev(f_lam, Xr).T, ev(f_amp, Xr), ev(f_noise, X)
    lamS, ampS = ev(f_lam, Xsr).T, ev(f_amp, Xsr)
    mX, mS = 0.3 * X[0], 0.3 * Xs[0]
    return X, y, Xs, lamX, ampX, noiX, lamS, ampS, mX, mS


@pytest.mark.parametrize("d,N,M,disc", [(1, 1, 2, None), (2, 50, 33, None), (8, 300, 70, None), (3, 1100, 40, None), (20, 200, 65, None),
                                        (3, 150, 50, [False, True, False])])
def test_nonstationary_gp_cov_parity(api, O, d, N, M, disc):
    X, y, Xs, lamX, ampX, noiX, lamS, ampS, mX, mS = gibbs_case(api, d, N, M, disc=disc)
    if M >= 3:
        Xs[:, 2] = Xs[:, 1]
        lamS[:, 2], ampS[2], mS[2] = lamS[:, 1], ampS[1], mS[1]
    post = O.nonstationary_fit(X, y, lamX, ampX, noiX, mean=mX, discrete=disc)
    mu_o, S_o, tol = gibbs_expected(O, post, Xs, lamS, ampS, mS, disc)
    g = api.GibbsGP(X, y, disc)
    g.update(lamX, ampX, noiX, mX)
    mu, S = g.predict_cov(Xs, lamS, ampS, mS)
    scale = ampS.max() ** 2
    assert np.array_equal(S, S.T) and np.isfinite(S).all()
    assert np.abs(S - clip_diag(O, S_o)).max() <= tol * scale, np.abs(S - clip_diag(O, S_o)).max()
    assert np.abs(mu - mu_o).max() <= tol * (1 + np.abs(mu_o).max())
    mu_p, var_p = g.predict(Xs, lamS, ampS, mS)
    assert np.abs(mu - mu_p).max() <= tol * (1 + np.abs(mu_p).max()) and np.abs(np.diag(S) - var_p).max() <= tol * scale
    assert np.diag(S).min() >= 0.0
    if M >= 3:
        assert np.abs(S[1] - S[2]).max() <= 1e-12 * scale
    g.close()


def test_nonstationary_cov_constant_latents_equal_the_plain_cov(api, O):
    """With constant latents the Gibbs kernel is the ARD squared-exponential kernel: the new entry point reproduces the shipped
    boss_gp_predict_cov (the plain model adds 1e-8 to its parameters)."""
    d, N, M = 4, 500, 300
    X, y, Xs = make(d, N, M, seed=6)
    lam, amp, sig = np.linspace(0.4, 0.9, d), 1.2, 0.05
    gp = api.GP(X, y, "sqexp")
    gp.update(lam - 1e-8, amp - 1e-8, sig - 1e-8)
    mu_p, S_p = gp.predict_cov(Xs)
    g = api.GibbsGP(X, y)
    g.update(np.tile(lam[:, None], (1, N)), np.full(N, amp), np.full(N, sig))
    mu, S = g.predict_cov(Xs, np.tile(lam[:, None], (1, M)), np.full(M, amp))
    assert np.allclose(mu, mu_p, rtol=0, atol=1e-9) and np.allclose(S, S_p, rtol=0, atol=1e-9)
    gp.close()
    g.close()


def test_nonstationary_cov_domain_error(api, O):
    """Well-separated points, a huge amplitude and a tiny noise, predicted at the training points: the diagonal of Σ falls below
    −1e-8 at rounding level (_clip_var's DomainError), in the oracle as on the device."""
    X = np.arange(0.0, 400.0, 10.0)[None, :]
    y = np.sin(X[0])
    N = X.shape[1]
    Xs = X.copy()
    lamX, ampX, noiX = np.full((1, N), 3.0), np.full(N, 1e5), np.full(N, 1e-4)
    post = O.nonstationary_fit(X, y, lamX, ampX, noiX)
    _, S_o, _ = gibbs_expected(O, post, Xs, lamX, ampX)
    with pytest.raises(O.DomainError):
        O.clip_var(np.diag(S_o))
    g = api.GibbsGP(X, y)
    g.update(lamX, ampX, noiX)
    with pytest.raises(api.DomainError) as e:
        g.predict_cov(Xs, lamX, ampX)
    assert e.value.code == api.BOSS_E_NEG_VAR and 0 <= e.value.bad_index < N
    g.close()


def test_cov_entry_points_validate_before_device_work(api, O):
    lib = api.load_library()
    d, n, N = 2, 12, 40
    X, y, dY = make_grad(d, n)
    gg = api.GradGP(X, y, dY, "matern52")
    Xn, yn, Xs = make(d, N, 10, seed=2)
    f_lam, f_amp, f_noise = latent(d)
    gn = api.GibbsGP(Xn, yn)
    lamS, ampS = ev(f_lam, Xs).T, ev(f_amp, Xs)
    with pytest.raises(api.BossError) as e:                  # not fitted yet
        gg.predict_value_cov(Xs)
    assert e.value.code == api.BOSS_E_NOT_FITTED
    with pytest.raises(api.BossError) as e:
        gn.predict_cov(Xs, lamS, ampS)
    assert e.value.code == api.BOSS_E_NOT_FITTED
    gg.update([0.5, 0.5], 1.0, 0.1, 0.1)
    gn.update(ev(f_lam, Xn).T, ev(f_amp, Xn), ev(f_noise, Xn))
    plain = api.fit(Xn, yn, "matern52", [0.5, 0.5], 1.0, 0.1)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    one = np.zeros(1)
    bad = C.c_long(0)
    Xf = np.asfortranarray(Xs)
    # wrong handle kinds, both ways (and the plain handle)
    assert lib.boss_ggp_predict_cov(gn._h, 10, dp(Xf), dp(np.zeros(10)), dp(np.zeros(100))) == api.BOSS_E_INVALID
    assert lib.boss_ggp_predict_cov(plain._h, 10, dp(Xf), dp(np.zeros(10)), dp(np.zeros(100))) == api.BOSS_E_INVALID
    lam_f, amp_f = np.asfortranarray(lamS), np.ascontiguousarray(ampS)
    for h in (gg._h, plain._h):
        assert lib.boss_ngp_predict_cov(h, 10, dp(Xf), dp(lam_f), dp(amp_f), None, dp(np.zeros(10)), dp(np.zeros(100)),
                                        C.byref(bad)) == api.BOSS_E_INVALID
    # NULL arguments
    assert lib.boss_ggp_predict_cov(gg._h, 10, None, dp(np.zeros(10)), dp(np.zeros(100))) == api.BOSS_E_INVALID
    assert lib.boss_ggp_predict_cov(gg._h, 10, dp(Xf), dp(np.zeros(10)), None) == api.BOSS_E_INVALID
    with pytest.raises(api.BossError) as e:
        gn.predict_cov(Xs)                                   # latents missing: the library's NULL check
    assert e.value.code == api.BOSS_E_INVALID
    # λ <= 0, α < 0
    with pytest.raises(api.BossError) as e:
        gn.predict_cov(Xs, np.where(np.arange(10) == 3, 0.0, lamS), ampS)
    assert e.value.code == api.BOSS_E_INVALID
    with pytest.raises(api.BossError) as e:
        gn.predict_cov(Xs, lamS, np.where(np.arange(10) == 5, -1.0, ampS))
    assert e.value.code == api.BOSS_E_INVALID
    # M < 1 and M above the cap: one-element outputs, nothing may be written before the check
    for M in (0, -3, 32769, 1 << 20):
        mu1, cov1 = np.full(1, 7.0), np.full(1, 7.0)
        assert lib.boss_ggp_predict_cov(gg._h, M, dp(Xf), dp(mu1), dp(cov1)) == api.BOSS_E_INVALID
        assert lib.boss_ngp_predict_cov(gn._h, M, dp(Xf), dp(lam_f), dp(amp_f), None, dp(mu1), dp(cov1), C.byref(bad)) == api.BOSS_E_INVALID
        assert mu1[0] == 7.0 and cov1[0] == 7.0
    # the handles still predict
    mu, S = gg.predict_value_cov(Xs)
    assert np.isfinite(S).all() and np.array_equal(S, S.T)
    mu, S = gn.predict_cov(Xs, lamS, ampS)
    assert np.isfinite(S).all() and np.array_equal(S, S.T)
    for h in (gg, gn, plain):
        h.close()


def test_cov_models_64_candidate_tiles():
    """BOSS_FORCE_BN64=1 (read once per process, hence the subprocess) puts V in 64-wide slabs for both models."""
    code = r'''
import sys, numpy as np, scipy.linalg as sla
sys.path.insert(0, %r)
from boss_jl_amd import api
from oracle import gp_oracle as O
rng = np.random.default_rng(3)
d, n, M = 3, 90, 150
X = rng.uniform(0, 1, (d, n)); y = np.sin(3 * X).sum(0); dY = 3 * np.cos(3 * X)
Xs = rng.uniform(0, 1, (d, M)); lam = np.full(d, 0.5)
post = O.gradient_gp_fit(X, y, dY, "matern52", lam, 1.0, 0.05, 0.1)
Ks = O.augmented_cross_cov("matern52", X, lam, 1.0, Xs)
V = sla.solve_triangular(post.L, Ks, lower=True)
S_o = (1.0 + 1e-8) ** 2 * O.kappa(O.KERNEL_NAMES["matern52"], O.scaled_distance(Xs, Xs, lam + 1e-8)) - V.T @ V
g = api.GradGP(X, y, dY, "matern52"); g.update(lam, 1.0, 0.05, 0.1)
mu, S = g.predict_value_cov(Xs)
assert np.array_equal(S, S.T) and np.allclose(S, S_o, rtol=0, atol=1e-8) and np.allclose(mu, Ks.T @ post.alpha, rtol=0, atol=1e-8)
N = 700
Xn = rng.uniform(0, 1, (d, N)); yn = np.sin(2 * np.pi * Xn).sum(0)
lamX, ampX, noiX = 0.3 + 0.2 * Xn, 1.0 + 0.3 * Xn[0], np.full(N, 0.05)
lamS, ampS = 0.3 + 0.2 * Xs, 1.0 + 0.3 * Xs[0]
op = O.nonstationary_fit(Xn, yn, lamX, ampX, noiX)
Ks = O.gibbs_kernel_matrix(Xn, lamX, ampX, Xs, lamS, ampS)
V = sla.solve_triangular(op.L, Ks, lower=True)
S_o = O.gibbs_kernel_matrix(Xs, lamS, ampS, Xs, lamS, ampS) - V.T @ V + 1e-18 * np.eye(M)
S_o[np.diag_indices(M)] = O.clip_var(np.diag(S_o))
h = api.GibbsGP(Xn, yn); h.update(lamX, ampX, noiX)
mu, S = h.predict_cov(Xs, lamS, ampS)
assert np.array_equal(S, S.T) and np.allclose(S, S_o, rtol=0, atol=1e-8) and np.allclose(mu, Ks.T @ op.a, rtol=0, atol=1e-8)
print("ok64")
''' % ROOT
    env = dict(os.environ, BOSS_FORCE_BN64="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok64" in r.stdout, r.stdout + r.stderr


def test_cov_models_host_mirror(api, O):
    import boss_jl_amd as B
    d, n, P, M = 3, 40, 2, 25
    X, y, dY = make_grad(d, n)
    Y, dYs = np.stack([y, 0.5 * y + 0.1]), np.stack([dY, 0.5 * dY])
    prm = B.HipGradientGPParams(np.array([[0.4, 0.5], [0.5, 0.6], [0.6, 0.7]]), np.array([1.1, 0.9]), np.array([0.05, 0.04]),
                                np.array([0.1, 0.12]))
    model = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P)
    post = model.model_posterior(prm, B.GradientData(X, Y, dYs))
    Xs = np.asfortranarray(np.random.default_rng(2).uniform(0, 1, (d, M)))
    mu, S = post.mean_and_cov(Xs)
    assert mu.shape == (P, M) and S.shape == (M, M, P)
    for i, s in enumerate(post.slices):
        mu_i, S_i = s.gp.predict_value_cov(Xs)
        assert np.array_equal(mu[i], mu_i) and np.array_equal(S[:, :, i], S_i) and np.array_equal(s.cov(Xs), S_i)
    for s in post.slices:
        s.close()
    f_lam, f_amp, f_noise = latent(2)
    Xn, yn, Xs2 = make(2, 60, 30, seed=7)
    ns = B.HipNonstationaryGP([f_lam], [f_amp], [f_noise], mean=[lambda x: 0.2 * x[0]])
    sl = ns.model_posterior_slice(B.ExperimentData(Xn, yn[None]), 0)
    mu, S = sl.mean_and_cov(Xs2)
    mu_v, var_v = sl.mean_and_var(Xs2)
    assert np.allclose(mu, mu_v, rtol=0, atol=1e-12) and np.allclose(np.diag(S), var_v, rtol=0, atol=1e-12)
    assert np.array_equal(sl.cov(Xs2), S)
    sl.close()
