"""GPU tests (pytest -m gpu) of the nonstationary likelihood in whitened latent parameters (boss_nfit_*; api.NgpWhitened,
HipNonstationaryModel, HipNonstationaryMAP) against the host reference chain and the case family of tests/test_nfit_host.py.

Shapes (N, d, S) = (37, 1, 3), (129, 2, 3), (200, 3, 3), (260, 2, 2): one past a 128 block / two 64-row tiles of the products; a
gradient step padded to 256; three lengthscale latents sharing a factor; two 256-row steps and a product whose K loop crosses tiles.
(129, 2, 3) once more with a prior mean at the data and one discrete dimension.

Bars, with u = 2⁻⁵³ and tol = max(1e-9, cond(K)·N·u·8) (the project's bar for the nonstationary likelihood and its cotangents):
 1. values:     |Δv_j| <= |v′_j|·8·N·u·(|L||θ| + |μ|)_j + 8u|v_j|      (the dot-product bound through the transform's derivative)
 2. twin:       ll, status == api.ngp_loglike_batch on values(theta)'s arrays, bit for bit
 3. pull-back:  with c_dev from api.ngp_loglike_grad_batch on those arrays and the REFERENCE v′,
                |g − L_fᵀ(c_dev ⊙ v′_ref)|_i <= 8·N·u·Σ_j |L_ji||c_dev_j v′_j| + Σ_j |L_ji||c_dev_j|·s_j,
                s_j = 8·N·u·(|L||θ| + |μ|)_j·10|v′_j| + 8u|v′_j|
                (s_j: the derivative evaluated at the device's L θ + μ instead of the reference's — the value bound's argument error
                times |v″| <= 10|v′|, which holds for every transform of the family: v″/v′ is p1 (lognormal), −m (uniform, |m| < 10),
                a sigmoid slope (softplus), 1 (exp) — plus the rounding of v′ itself);  a scalar latent: |g − Σ_j c_dev_j| <= N·u·Σ|c_dev|
 4. chain:      |Δℓ| <= tol (1 + |ℓ|),   max|Δg| <= 100·tol·(1 + max|c_oracle|)·max(1, A),   A = max_{q,i} Σ_j |L_ji||v′_j|
                (the cotangent bar times the pull-back's amplification, both from the reference)

Run as a script (`python tests/test_gpu_nfit.py <out.npz>`) the module evaluates the child case in a fresh process: the chunk and
poisoned-allocation tests start it with their environment switch set."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_nfit_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SHAPES = [(37, 1, 3), (129, 2, 3), (200, 3, 3), (260, 2, 2)]


@pytest.fixture(scope="module")
def api():
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def B(api):
    import boss_jl_amd
    return boss_jl_amd


def handle(api, c):
    return api.NgpWhitened(c.X, c.y, c.factors, c.factor_of, c.specs, c.mu, mean_X=c.mean_X, discrete=c.discrete)


_cache = {}


def reference(B, key):
    """The case and its host reference, computed once per shape and shared: per set the values, derivative, bounds, ℓ, gradient,
    cotangents, cond(K)."""
    if key in _cache:
        return _cache[key]
    N, d, S, scalar = key[:4]
    c = H.family(N, d, S, scalar=scalar, **dict(key[4:]))          # (further entries: (name, value) pairs of the family's options)
    r = H.Case()
    r.v, r.dv, r.bnd, r.ll, r.g, r.cot, r.cond = [], [], [], [], [], [], []
    for s in range(S):
        v, dv, _, bnd = H.ref_values(B, c, c.theta[:, s])
        ll, g, cot, _ = H.ref_chain(B, c, c.theta[:, s])
        Xr = H.O.discrete_round(c.X, c.discrete)
        K = H.O.gibbs_kernel_matrix(Xr, v[:d], v[d], Xr, v[:d], v[d]) + np.diag(v[d + 1] ** 2)
        r.v.append(v), r.dv.append(dv), r.bnd.append(bnd), r.ll.append(ll), r.g.append(g), r.cot.append(cot), r.cond.append(np.linalg.cond(K))
    _cache[key] = (c, r)
    return c, r


def check_all_bars(api, B, key):
    c, r = reference(B, key)
    N, d, S = c.N, c.d, c.S
    h = handle(api, c)
    try:
        lam, amp, noi, stv = h.values(c.theta)
        ll, st, g = h.loglike_grad(c.theta)
        ll0, st0, g0 = h.loglike_grad(c.theta, want_grad=False)
    finally:
        h.close()
    assert not stv.any() and not st.any() and g0 is None
    # 2. the array twin
    ll_t, st_t = api.ngp_loglike_batch(c.X, c.y, lam, amp, noi, mean_X=c.mean_X, discrete=c.discrete)
    assert np.array_equal(ll, ll_t) and np.array_equal(st, st_t) and np.array_equal(ll0, ll_t) and np.array_equal(st0, st_t)
    res = api.ngp_loglike_grad_batch(c.X, c.y, lam, amp, noi, mean_X=c.mean_X, discrete=c.discrete)
    assert np.array_equal(res[0], ll)
    for s in range(S):
        v_dev = np.vstack([lam[:, :, s], amp[None, :, s], noi[None, :, s]])
        # 1. values
        bound = np.abs(r.dv[s]) * 8 * N * U * r.bnd[s] + 8 * U * np.abs(r.v[s])
        err = np.abs(v_dev - r.v[s])
        print(f"values {key} set {s}: max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert (err <= bound).all(), (key, s, float(np.max(err / np.maximum(bound, 1e-300))))
        # 3. the pull-back alone
        c_dev = np.vstack([res[2][:, :, s], res[3][None, :, s], res[4][None, :, s]])
        want = H.pull_back(c, c_dev, r.dv[s])
        for q in range(d + 2):
            f = c.factor_of[q]
            if f < 0:
                e, b = abs(g[c.off[q], s] - want[c.off[q]]), N * U * np.abs(c_dev[q]).sum()
                print(f"scalar pull-back {key} set {s} latent {q}: err {e:.3g} bound {b:.3g}")
                assert e <= b, (key, s, q, e, b)
                continue
            aL = np.abs(c.factors[f])
            slack = 8 * N * U * r.bnd[s][q] * 10 * np.abs(r.dv[s][q]) + 8 * U * np.abs(r.dv[s][q])
            b = 8 * N * U * (aL.T @ np.abs(c_dev[q] * r.dv[s][q])) + aL.T @ (np.abs(c_dev[q]) * slack)
            e = np.abs(g[c.off[q]:c.off[q] + N, s] - want[c.off[q]:c.off[q] + N])
            print(f"pull-back {key} set {s} latent {q}: max err/bound {np.max(e / np.maximum(b, 1e-300)):.3g}")
            assert (e <= b).all(), (key, s, q, float(np.max(e / np.maximum(b, 1e-300))))
        # 4. the whole chain
        tol = max(1e-9, r.cond[s] * N * U * 8)
        A = max(float(np.max(np.abs(c.factors[c.factor_of[q]]).T @ np.abs(r.dv[s][q]))) for q in range(d + 2) if c.factor_of[q] >= 0)
        gbar = 100 * tol * (1 + np.abs(r.cot[s]).max()) * max(1.0, A)
        print(f"chain {key} set {s}: cond {r.cond[s]:.3g} dll {abs(ll[s] - r.ll[s]):.3g} (bar {tol * (1 + abs(r.ll[s])):.3g}) "
              f"dg {np.abs(g[:, s] - r.g[s]).max():.3g} (bar {gbar:.3g})")
        assert abs(ll[s] - r.ll[s]) <= tol * (1 + abs(r.ll[s])), (key, s)
        assert np.abs(g[:, s] - r.g[s]).max() <= gbar, (key, s)
    return c, g


# ------------------------------------------------------------------------------------------ 1-4. the bars, shape by shape
@pytest.mark.parametrize("N,d,S", SHAPES)
def test_values_twin_pull_back_and_chain(api, B, N, d, S):
    check_all_bars(api, B, (N, d, S, ()))


# ------------------------------------------------------------------------------------------ 5. scalar latents
def test_scalar_latents(api, B):
    c, g = check_all_bars(api, B, (129, 2, 3, (1, 3)))
    assert c.T == 2 * 129 + 2 and g.shape == (c.T, 3)
    h = handle(api, c)
    lam, amp, noi, _ = h.values(c.theta)
    h.close()
    assert (lam[1] == 0.4).all() and (noi == 0.1).all()            # taken as given, at every point


def test_prior_mean_and_discrete_dimension(api, B):
    """NgpWhitened(mean_X=…, discrete=…) at (129, 2, 3): a prior mean at the data and the second dimension rounded inside the kernel
    (five levels), through every bar of the module docstring; the reference chain carries both (tests/test_nfit_host.py), and the
    likelihood is neither that of the handle without the mean nor that of the handle without the rounding."""
    key = (129, 2, 3, (), ("mean", True), ("discrete", (False, True)))
    c, g = check_all_bars(api, B, key)
    assert c.mean_X is not None and c.discrete.tolist() == [False, True] and np.isfinite(g).all()
    _, r = reference(B, key)
    for drop in ("mean_X", "discrete"):
        kw = dict(mean_X=c.mean_X, discrete=c.discrete)
        kw[drop] = None
        h = api.NgpWhitened(c.X, c.y, c.factors, c.factor_of, c.specs, c.mu, **kw)
        try:
            ll, st, _ = h.loglike_grad(c.theta, want_grad=False)
        finally:
            h.close()
        assert not st.any() and (np.abs(ll - np.array(r.ll)) > 1e-3).all(), (drop, ll, r.ll)


# ------------------------------------------------------------------------------------------ 6. position independence, determinism
def test_position_independence_and_determinism(api, B):
    c = H.family(129, 2, 5, seed=2)
    h = handle(api, c)
    try:
        ll, st, g = h.loglike_grad(c.theta)
        ll2, st2, g2 = h.loglike_grad(c.theta)
        assert not st.any() and np.array_equal(ll, ll2) and np.array_equal(g, g2) and np.array_equal(st, st2)
        v = h.values(c.theta)
        for s in range(5):                                           # alone
            l1, s1, g1 = h.loglike_grad(c.theta[:, s:s + 1])
            assert l1[0] == ll[s] and np.array_equal(g1[:, 0], g[:, s]), s
            v1 = h.values(c.theta[:, s:s + 1])
            assert all(np.array_equal(a[..., 0], b[..., s]) for a, b in zip(v1[:3], v[:3])), s
        perm = np.array([3, 0, 4, 2, 1])
        lp, sp, gp = h.loglike_grad(c.theta[:, perm])
        assert np.array_equal(lp, ll[perm]) and np.array_equal(gp, g[:, perm])
    finally:
        h.close()
    # one shared factor against the same factor uploaded twice under two indices
    one = api.NgpWhitened(c.X, c.y, [c.factors[0]], [0, 0, 0, 0], c.specs, c.mu)
    two = api.NgpWhitened(c.X, c.y, [c.factors[0], c.factors[0].copy()], [0, 1, 1, 0], c.specs, c.mu)
    try:
        a, b = one.loglike_grad(c.theta), two.loglike_grad(c.theta)
        assert not a[1].any() and all(np.array_equal(x, y) for x, y in zip(a, b))
    finally:
        one.close()
        two.close()


# ------------------------------------------------------------------------------------------ 7. chunks, poisoned memory
def child_case(api):
    c = H.family(129, 2, 3, scalar=(1,))
    h = handle(api, c)
    ll, st, g = h.loglike_grad(c.theta)
    lam, amp, noi, stv = h.values(c.theta)
    ll0, st0, _ = h.loglike_grad(c.theta, want_grad=False)
    h.close()
    return ll, st, g, lam, amp, noi, stv, ll0, st0


def run_child(env_extra, tmp_path):
    out = os.path.join(str(tmp_path), "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, **env_extra), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return np.load(out)


@pytest.fixture(scope="module")
def plain_child_case(api):
    return child_case(api)


def test_chunked_call_agrees_bitwise(api, plain_child_case, tmp_path):
    """BOSS_MODEL_BATCH_CHUNK_MB=0 (read once per process, so in a child): the limit holds no matrix, and a chunk is never less than
    one set — every set is a chunk of its own whatever the padded size, so the three sets go in three chunks."""
    child = run_child({"BOSS_MODEL_BATCH_CHUNK_MB": "0"}, tmp_path)
    for k, want in enumerate(plain_child_case):
        assert np.array_equal(child[f"a{k}"], want), k


def test_poisoned_allocations(api, plain_child_case, tmp_path):
    """Every new device allocation filled with NaN patterns: what the products, the transform and the gradient pass read of
    factors, chunk buffers and parameter blocks must all have been written by the call."""
    child = run_child({"BOSS_POISON_ALLOC": "1"}, tmp_path)
    for k, want in enumerate(plain_child_case):
        assert np.array_equal(child[f"a{k}"], want), k


# ------------------------------------------------------------------------------------------ 8. failures stay local
def test_failures_stay_local(api, B):
    c = H.family(129, 2, 5, seed=3, scalar=(1,))
    good = [0, 2, 4]
    th = c.theta.copy(order="F")
    th[c.off[2] + 7, 1] = np.nan                                    # a NaN in an amplitude latent's yϵ
    th[c.off[1], 3] = -1.0                                           # the scalar lengthscale
    h = handle(api, c)
    try:
        ll, st, g = h.loglike_grad(th)
        assert st.tolist() == [0, api.BOSS_E_INVALID, 0, api.BOSS_E_INVALID, 0], st
        assert ll[1] == -np.inf and ll[3] == -np.inf and not g[:, 1].any() and not g[:, 3].any()
        lg, sg, gg = h.loglike_grad(th[:, good])
        assert not sg.any() and np.array_equal(ll[good], lg) and np.array_equal(g[:, good], gg) and np.isfinite(gg).all()
        assert h.values(th)[3].tolist() == st.tolist()
        l0, s0, _ = h.loglike_grad(th, want_grad=False)
        assert np.array_equal(l0, ll) and np.array_equal(s0, st)
    finally:
        h.close()
    # two coincident points and scalar noise 0: whatever the array twin reports on the same values
    c = H.family(37, 1, 2, seed=4, scalar=(2,), scalar_values={2: 0.0})
    c.X[:, 1] = c.X[:, 0]
    h = handle(api, c)
    try:
        ll, st, g = h.loglike_grad(c.theta)
        lam, amp, noi, _ = h.values(c.theta)
    finally:
        h.close()
    ll_t, st_t = api.ngp_loglike_batch(c.X, c.y, lam, amp, noi)
    assert np.array_equal(st, st_t) and np.array_equal(ll, ll_t)
    for s in range(2):
        assert st[s] == api.BOSS_OK or not g[:, s].any()


# ------------------------------------------------------------------------------------------ 9. the model layer
def _model(B, d):
    """The family's latent models with narrower targets (0.2 in place of 0.3 / 0.4): the kernel's (α_i + α_j)/2 prefactor is not
    positive definite for every amplitude function, and with the family's widths the third FULL-scale prior draw of seed 0 (the
    family itself uses 0.5·N(0, 1)) has a negative eigenvalue (−0.013 at N = 60; checked with the oracle); with 0.2 the three draws
    have λ_min >= 0.008, cond(K) <= 6.3e3."""
    from scipy import stats
    lam_gp = B.HipParametrizedGP([0.4] * d, "matern32", stats.lognorm(s=0.2, scale=0.3), B.identity_act, noise_std=1e-2)
    amp_gp = B.HipParametrizedGP([0.7] * d, "matern52", stats.norm(0.5, 0.2), B.softplus.with_lower_bound(0.2), noise_std=1e-2)
    return B.HipNonstationaryModel(lengthscale_models=[[lam_gp] * d], amplitude_models=[amp_gp], noise_std_models=[B.LogNormal(-2.3, 0.3)])


def test_model_layer_equals_the_api_call(api, B):
    c = H.family(60, 1, 3, seed=5)
    model = _model(B, 1)
    data = B.ExperimentData(c.X, c.y[None, :])
    sample = model.params_sampler(data)
    rng = np.random.default_rng(0)
    plist = [sample(rng) for _ in range(3)]
    p0 = plist[0]
    assert plist[1].lam[0][0].L is p0.lam[0][0].L                    # one factor for all draws
    tot, G = model.data_loglike_grad_batch(data, plist)
    vec, _ = model.vectorizer(data)
    Th = np.stack([vec(p) for p in plist], axis=1)
    assert Th.shape == (2 * 60 + 1, 3)
    h = api.NgpWhitened(c.X, c.y, [p0.lam[0][0].L, p0.amp[0].L], [0, 1, -1],
                        [model.lengthscale_models[0][0].device_spec(), model.amplitude_models[0].device_spec(), None])
    ll, st, g = h.loglike_grad(Th)
    h.close()
    assert not st.any() and np.array_equal(tot, ll) and np.array_equal(G, g)
    assert np.array_equal(model.data_loglike_batch(data, plist), ll)
    model.close()


def test_map_ascends_and_the_fitted_model_predicts(api, B):
    c = H.family(60, 1, 1, seed=6)
    model = _model(B, 1)
    data = B.ExperimentData(c.X, c.y[None, :])
    prob = B.BossProblem(None, B.Domain((np.zeros(1), np.ones(1))), B.ExpectedImprovement(B.LinFitness([1.0])), model, data)
    fitter = B.HipNonstationaryMAP(multistart=3, iters=5, seed=0)
    allr = fitter.estimate_parameters(prob, return_all=True)
    hist = fitter.history
    assert len(allr) == 3 and len(hist) == 3
    for k in range(3):
        assert all(b > a for a, b in zip(hist[k], hist[k][1:])) and allr[k].loglike == hist[k][-1], hist[k]
    assert any(len(hk) > 1 for hk in hist)
    best = B.HipNonstationaryMAP(multistart=3, iters=5, seed=0).estimate_parameters(prob)
    assert best.loglike == max(r.loglike for r in allr) and all(best.loglike >= hk[0] for hk in hist)
    # the returned value is the log-posterior at the returned parameters
    tot, _ = model.data_loglike_grad_batch(data, [best.params])
    assert abs(tot[0] + model.params_loglike(data)(best.params) - best.loglike) <= 1e-9 * (1 + abs(best.loglike))
    slices = model.model_posterior(best.params, data)
    try:
        Xs = np.linspace(0.02, 0.98, 16)[None, :]
        mu, var = slices[0].mean_and_var(Xs)
        assert mu.shape == (16,) and np.isfinite(mu).all() and np.isfinite(var).all() and (var >= 0).all()
    finally:
        for s in slices:
            s.close()
        model.close()


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api as _api
    np.savez(sys.argv[1], **{f"a{k}": a for k, a in enumerate(child_case(_api))})
