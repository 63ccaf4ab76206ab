"""The nonstationary likelihood in whitened latent parameters (boss_nfit_*), the parts that need no device: the host reference
chain of the feature against central finite differences, the model layer's vectoriser and prior, and the argument checks.

Reference chain (what tests/test_gpu_nfit.py compares the device against).  Per latent q with factor f and spec_q
    v_q, v′_q = nonstationary.latent_transform(spec_q, L_f θ_q + μ_q),
then (ℓ, dlam, damp, dnoise, _) = oracle.gp_oracle.nonstationary_loglike_grad(X, y, v[:d], v[d], v[d+1], mean, discrete) and
    g_q = L_fᵀ (c_q ⊙ v′_q),      c = (dlam rows, damp, dnoise);        a scalar latent: v_q = θ_q at every point, g_q = Σ_j c_q[j].

Case family: X ~ U(0,1)^{d×N}, y = Σ sin(2πx)/√d + 0.05 ε; factor 0 = the oracle's Cholesky factor of a matern32 prior (λ = 0.4,
amplitude 1, noise 1e-2) for the lengthscale latents, factor 1 = matern52, λ = 0.7 for amplitude and noise; even lengthscale
dimensions lognormal(log 0.3, 0.3), odd ones uniform(0.15, 0.6), identity activation; amplitude normal(0.5, 0.4) -> softplus + 0.2;
noise: no target, exp, μ = −1.5; θ = 0.5·N(0, 1)."""
import math

import numpy as np
import pytest

import __graft_entry__ as entry
from oracle import gp_oracle as O


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    return a


@pytest.fixture(scope="module")
def B(api):
    import boss_jl_amd
    return boss_jl_amd


# ------------------------------------------------------------------------------------------ the case family and the chain
class Case:
    pass


def family(N, d, S, seed=0, scalar=(), scalar_values=None, mean=False, discrete=None):
    """The family of the module docstring.  scalar: latent indices q that are scalar latents (their value: scalar_values[q],
    default 0.4 for a lengthscale, 1.0 amplitude, 0.1 noise).  mean: the prior mean m(x) = 0.3 + 0.2 Σx at the data (c.mean_X, else
    None).  discrete: per-dimension flags (c.discrete, else None); the flagged coordinates are stretched to [0, 4] so that the
    kernel's rounding yields five levels (y, the factors and theta are those of the unstretched family: the same random stream)."""
    rng = np.random.default_rng(1000 + 17 * N + d + seed)
    c = Case()
    c.N, c.d, c.S = N, d, S
    c.X = rng.uniform(0, 1, (d, N))
    c.y = np.sin(2 * np.pi * c.X).sum(0) / math.sqrt(d) + 0.05 * rng.standard_normal(N)
    c.factors = [O.gp_fit(c.X, np.zeros(N), "matern32", np.full(d, 0.4), 1.0, 1e-2).L,
                 O.gp_fit(c.X, np.zeros(N), "matern52", np.full(d, 0.7), 1.0, 1e-2).L]
    c.factors = [np.asfortranarray(np.tril(L)) for L in c.factors]
    c.specs = [("lognormal", (math.log(0.3), 0.3), "identity", 0.0) if l % 2 == 0 else ("uniform", (0.15, 0.6), "identity", 0.0)
               for l in range(d)] + [("normal", (0.5, 0.4), "softplus", 0.2), ("none", (0.0, 0.0), "exp", 0.0)]
    c.mean_X, c.discrete = None, None
    if discrete is not None:
        c.discrete = np.asarray(discrete, dtype=bool)
        c.X = np.asfortranarray(np.where(c.discrete[:, None], 4.0 * c.X, c.X))
    if mean:
        c.mean_X = 0.3 + 0.2 * c.X.sum(0)
    c.factor_of = [0] * d + [1, 1]
    c.mu = np.zeros((N, d + 2), order="F")
    c.mu[:, d + 1] = -1.5
    defaults = [0.4] * d + [1.0, 0.1]
    for q in scalar:
        c.factor_of[q] = -1
        c.specs[q] = None
    c.off, c.T = [], 0
    for q in range(d + 2):
        c.off.append(c.T)
        c.T += N if c.factor_of[q] >= 0 else 1
    c.theta = np.zeros((c.T, S), order="F")
    for q in range(d + 2):
        if c.factor_of[q] >= 0:
            c.theta[c.off[q]:c.off[q] + N] = 0.5 * rng.standard_normal((N, S))
        else:
            c.theta[c.off[q]] = (scalar_values or {}).get(q, defaults[q])
    return c


def ref_values(B, c, th):
    """v [d+2, N], v′ [d+2, N], m = Lθ + μ [d+2, N], and the dot-product bound (|L||θ| + |μ|) [d+2, N] of one column of theta
    (scalar latents: v = θ, v′ = 1, bound 0)."""
    N, nq = c.N, c.d + 2
    v, dv, m, bnd = np.zeros((nq, N)), np.ones((nq, N)), np.zeros((nq, N)), np.zeros((nq, N))
    for q in range(nq):
        f = c.factor_of[q]
        if f < 0:
            v[q] = th[c.off[q]]
            continue
        t = th[c.off[q]:c.off[q] + N]
        m[q] = c.factors[f] @ t + c.mu[:, q]
        bnd[q] = np.abs(c.factors[f]) @ np.abs(t) + np.abs(c.mu[:, q])
        v[q], dv[q] = B.latent_transform(c.specs[q], m[q])
    return v, dv, m, bnd


def pull_back(c, cot, dv):
    """g = L_fᵀ (c_q ⊙ v′_q) per GP latent, Σ_j c_q[j] per scalar latent: cot, dv [d+2, N] -> g [T]."""
    g = np.zeros(c.T)
    for q in range(c.d + 2):
        f = c.factor_of[q]
        if f < 0:
            g[c.off[q]] = cot[q].sum()
        else:
            g[c.off[q]:c.off[q] + c.N] = c.factors[f].T @ (cot[q] * dv[q])
    return g


def ref_chain(B, c, th):
    """(ℓ, g [T], cotangents [d+2, N], v′) of one column of theta through the oracle."""
    v, dv, _, _ = ref_values(B, c, th)
    ll, dlam, damp, dnoise, _ = O.nonstationary_loglike_grad(c.X, c.y, v[:c.d], v[c.d], v[c.d + 1], mean=c.mean_X, discrete=c.discrete)
    cot = np.vstack([dlam, damp[None], dnoise[None]])
    return ll, pull_back(c, cot, dv), cot, dv


def ref_loglike(B, c, th):
    v = ref_values(B, c, th)[0]
    return O.nonstationary_fit(c.X, c.y, v[:c.d], v[c.d], v[c.d + 1], mean=c.mean_X, discrete=c.discrete).logpdf


# ------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("N,d", [(37, 1), (129, 2)])
def test_reference_chain_agrees_with_central_differences(B, N, d):
    """The chain the GPU tests use as their reference is itself checked: 12 random coordinates and the steepest direction against
    central differences.  Bar 1e-6·max(1, max|g|): with h = 1e-5 the truncation error is h²|ℓ‴|/6 and the rounding error of the
    difference u·|ℓ|·cond/h ≈ 1e-16·1e2·1e4/1e-5 = 1e-5·1e-2 at worst for this family (cond(K) <= 1.5e4, |ℓ| ~ 1e2) — the family was
    chosen so that chain and differences agree to 4e-8 relative, and the bar leaves that a factor 25."""
    c = family(N, d, 1)
    th = c.theta[:, 0]
    ll, g, _, _ = ref_chain(B, c, th)
    assert np.isfinite(ll) and np.isfinite(g).all()
    rng = np.random.default_rng(5)
    dirs = [np.eye(c.T)[k] for k in rng.choice(c.T, 12, replace=False)] + [g / np.linalg.norm(g)]
    h = 1e-5
    for u in dirs:
        fd = (ref_loglike(B, c, th + h * u) - ref_loglike(B, c, th - h * u)) / (2 * h)
        assert abs(fd - g @ u) <= 1e-6 * max(1.0, np.abs(g).max()), (fd, g @ u)


def test_reference_chain_with_prior_mean_and_discrete_dimension(B):
    """The family member tests/test_gpu_nfit.py passes to NgpWhitened(mean_X=…, discrete=…): the chain through the oracle's prior mean
    and rounding against central differences, by the bar of the test above; and both arguments change the likelihood."""
    c = family(37, 2, 1, mean=True, discrete=(False, True))
    assert c.mean_X.shape == (37,) and c.X[1].max() > 1.0 and len(np.unique(np.rint(c.X[1]))) == 5
    th = c.theta[:, 0]
    ll, g, _, _ = ref_chain(B, c, th)
    rng = np.random.default_rng(6)
    h = 1e-5
    for u in [np.eye(c.T)[k] for k in rng.choice(c.T, 12, replace=False)] + [g / np.linalg.norm(g)]:
        fd = (ref_loglike(B, c, th + h * u) - ref_loglike(B, c, th - h * u)) / (2 * h)
        assert abs(fd - g @ u) <= 1e-6 * max(1.0, np.abs(g).max()), (fd, g @ u)
    for change in (dict(mean_X=None), dict(discrete=None)):
        c2 = family(37, 2, 1, mean=True, discrete=(False, True))
        vars(c2).update(change)
        assert abs(ref_loglike(B, c2, th) - ll) > 1e-3


def test_reference_chain_scalar_latents(B):
    c = family(37, 2, 1, scalar=(1, 3))
    th = c.theta[:, 0]
    assert c.T == 2 * 37 + 2
    ll, g, cot, _ = ref_chain(B, c, th)
    h = 1e-6
    for q in (1, 3):
        u = np.zeros(c.T)
        u[c.off[q]] = 1.0
        fd = (ref_loglike(B, c, th + h * u) - ref_loglike(B, c, th - h * u)) / (2 * h)
        assert abs(fd - g[c.off[q]]) <= 1e-5 * max(1.0, abs(fd)), (q, fd, g[c.off[q]])


def test_symbols_are_declared_exported_and_bound(api, B):
    lib = api.load_library()
    for name in ("boss_nfit_create", "boss_nfit_free", "boss_nfit_param_count", "boss_nfit_values", "boss_nfit_loglike_grad"):
        assert hasattr(lib, name) and name in api.SIGNATURES, name
    for name in ("NgpWhitened", "HipNonstationaryModel", "HipNonstationaryParams", "HipNonstationaryMAP"):
        assert hasattr(B, name), name


def _no_device(api):
    return api.device_count() < 1


def test_without_a_device_create_fails_loudly_and_bad_arguments_come_first(api):
    c = family(12, 2, 1)
    args = lambda: dict(X=c.X, y=c.y, factors=c.factors, factor_of=list(c.factor_of), specs=list(c.specs), mu=c.mu)   # noqa: E731
    for change, what in ((dict(factor_of=[0, 0, 1, 2]), "factor_of"), (dict(factor_of=[0, -2, 1, 1]), "factor_of"),
                         (dict(specs=[c.specs[0], c.specs[1], (7, (0.0, 1.0), "identity", 0.0), c.specs[3]]), "target"),
                         (dict(specs=[c.specs[0], c.specs[1], c.specs[2], ("none", (0.0, 0.0), 5, 0.0)]), "activation")):
        with pytest.raises(api.BossError) as e:
            api.NgpWhitened(**dict(args(), **change))
        assert e.value.code == api.BOSS_E_INVALID and what in str(e.value), (what, str(e.value))
    c17 = family(8, 17, 1)
    with pytest.raises(api.BossError) as e:
        api.NgpWhitened(c17.X, c17.y, c17.factors, c17.factor_of, c17.specs, c17.mu)
    assert e.value.code == api.BOSS_E_INVALID and "16" in str(e.value)
    if _no_device(api):
        with pytest.raises(api.BossError) as e:
            api.NgpWhitened(**args())
        assert e.value.code == api.BOSS_E_NO_DEVICE


def _model_and_params(B, N=9, d=2):
    from scipy import stats
    from boss_jl_amd.nonstationary import HipParametrizedGPParams
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (d, N))
    data = B.ExperimentData(X, np.stack([np.sin(X[0]), np.cos(X[1])]))
    lam_gp = B.HipParametrizedGP([0.4] * d, "matern32", stats.lognorm(s=0.3, scale=0.3), B.identity_act)
    amp_gp = B.HipParametrizedGP([0.7] * d, "matern52", stats.norm(0.5, 0.4), B.softplus.with_lower_bound(0.2))
    model = B.HipNonstationaryModel(lengthscale_models=[[lam_gp, B.LogNormal(-1.0, 0.3)], [B.Dirac(0.5), lam_gp]],
                                    amplitude_models=[amp_gp, B.LogNormal(0.0, 0.2)], noise_std_models=[B.LogNormal(-2.0, 0.3), B.Dirac(0.1)])
    L0, L1, mu = np.tril(rng.standard_normal((N, N))), np.tril(rng.standard_normal((N, N))), np.zeros(N)
    gp = lambda L: HipParametrizedGPParams(data.X, mu, L, rng.standard_normal(N), np.full(d, 0.4))   # noqa: E731
    params = B.HipNonstationaryParams(lam=[[gp(L0), 0.37], [0.5, gp(L0)]], amp=[gp(L1), 1.1], noise=[0.12, 0.1])
    return model, data, params


def test_model_vectoriser_round_trip_and_prior(B):
    model, data, p = _model_and_params(B)
    N = data.X.shape[1]
    vec, devec = model.vectorizer(data)
    v = vec(p)
    assert v.shape == (3 * N + 5,)
    # all λ latents output after output, then α, then σ (nonstationary_gp.jl:302-330)
    assert np.array_equal(v[:N], p.lam[0][0].yeps) and v[N] == 0.37 and v[N + 1] == 0.5 and np.array_equal(v[N + 2:2 * N + 2], p.lam[1][1].yeps)
    assert np.array_equal(v[2 * N + 2:3 * N + 2], p.amp[0].yeps) and v[3 * N + 2] == 1.1 and v[3 * N + 3] == 0.12 and v[3 * N + 4] == 0.1
    q = devec(p, v)
    assert np.array_equal(vec(q), v) and q.lam[0][0].L is p.lam[0][0].L and q.amp[1] == 1.1
    w = v + 0.25
    assert np.array_equal(vec(devec(p, w)), w)
    # params_loglike: N(0, I) on every yϵ plus the scalar priors' logpdfs (nonstationary_gp.jl:250-279)
    want = sum(-0.5 * (x.yeps @ x.yeps) - 0.5 * N * math.log(2 * math.pi) for x in (p.lam[0][0], p.lam[1][1], p.amp[0]))
    want += B.LogNormal(-1.0, 0.3).logpdf(0.37) + 0.0 + B.LogNormal(0.0, 0.2).logpdf(1.1) + B.LogNormal(-2.0, 0.3).logpdf(0.12) + 0.0
    assert abs(model.params_loglike(data)(p) - want) <= 1e-12 * abs(want)


def test_model_refuses_a_transform_the_device_does_not_know(B):
    from scipy import stats
    bad = B.HipParametrizedGP([0.4], "matern32", stats.gamma(2.0), B.identity_act)
    ok = B.HipParametrizedGP([0.4], "matern32", None, B.exp_act)
    with pytest.raises(ValueError, match="is not one the device evaluates"):
        B.HipNonstationaryModel(lengthscale_models=[[ok]], amplitude_models=[bad], noise_std_models=[B.Dirac(0.1)])


def test_map_refuses_starts_with_different_factors(B):
    """The device keeps one whitening for all starts: given starts whose L differ must not be scored with start 0's (no device needed:
    the check comes first)."""
    from boss_jl_amd.nonstationary import HipParametrizedGPParams
    model, data, p = _model_and_params(B)
    x = p.amp[0]
    q = B.HipNonstationaryParams(lam=p.lam, amp=[HipParametrizedGPParams(x.X, x.mu, x.L * 1.5, x.yeps, x.lengthscale), p.amp[1]], noise=p.noise)
    prob = B.BossProblem(None, B.Domain((np.zeros(2), np.ones(2))), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])), model, data)
    with pytest.raises(ValueError, match="does not share the factors"):
        B.HipNonstationaryMAP(iters=1, starts=[p, q]).estimate_parameters(prob)
