"""GPU tests (pytest -m gpu) of the batched likelihoods of the gradient-observation and the nonstationary model:
boss_ggp_loglike_batch / boss_ngp_loglike_batch against the CPU oracle, against the single-handle updates, their determinism
and position independence, local failures, the model layer above them, and poisoned memory.

Tolerance: the project's rule (tests/test_gpu_parity.py) with cond(K) computed from the oracle's matrix —
    |Δll| <= 1e-9 (1 + |ll|)  for cond(K) <= 1e6,   cond(K)·N·2⁻⁵³·8 · (1 + |ll|)  beyond that.

Run as a script (`python tests/test_gpu_model_batch.py <case> <out.npz>`) the module evaluates one named case in a fresh
process: the poisoned-allocation and the two-chunk tests start it with their environment switch set.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
KERNELS = ("matern32", "matern52", "sqexp")


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


def ll_tol(cond, N):
    return 1e-9 if cond <= 1e6 else cond * N * 2.0 ** -53 * 8


# ------------------------------------------------------------------------------------------ cases
def grad_case(n, d, S, seed=0, dup=False):
    """y = sin(Xᵀw) with its exact gradient; S draws λ ∈ [0.3, 1.5], α ∈ [0.5, 2], σ, σ_∂ ∈ [0.05, 0.3]."""
    rng = np.random.default_rng(100 + seed)
    X = rng.uniform(0, 1, (d, n))
    if dup:
        X[:, 1] = X[:, 0]                                       # two coincident points: the entries evaluated at x_j + 1e-8
    w = rng.uniform(0.5, 2.0, d)
    y = np.sin(X.T @ w)
    dY = w[:, None] * np.cos(X.T @ w)[None, :]
    lam = rng.uniform(0.3, 1.5, (d, S))
    amp, sig, sgd = rng.uniform(0.5, 2.0, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
    return X, y, dY, lam, amp, sig, sgd


def grad_oracle(O, X, y, dY, kernel, lam, amp, sig, sgd):
    """Per set (logpdf, cond(K)) of the oracle; every set must factorise."""
    out = []
    for s in range(lam.shape[1]):
        post = O.gradient_gp_fit(X, y, dY, kernel, lam[:, s], amp[s], sig[s], sgd[s])
        assert np.isfinite(post.logpdf)
        out.append((post.logpdf, np.linalg.cond(post.L @ post.L.T)))
    return np.array(out).T


def latent(d):
    """The latent family of tests/test_gpu_parity.py::latent."""
    f_lam = lambda x: 0.25 + 0.5 * np.asarray(x) ** 2 + 0.1 * np.arange(1, d + 1)        # noqa: E731
    f_amp = lambda x: 1.0 + 0.4 * np.sin(3 * x[0])                                        # noqa: E731
    f_noise = lambda x: 0.03 + 0.05 * x[-1] ** 2                                           # noqa: E731
    return f_lam, f_amp, f_noise


def ns_case(d, N, S, seed=4, disc=None):
    """The data of test_gpu_parity.make(seed=4) (scaled to [0, 3] with a discrete dimension, so that rounding matters); S sets of
    the latent family scaled by c ∈ [0.7, 1.6] (λ), a ∈ [0.6, 1.8] (α), n ∈ [1, 3] (σ)."""
    rng = np.random.default_rng(seed)
    scale = 1.0 if disc is None else 3.0
    X = rng.uniform(0, scale, (d, N))
    y = np.sin(2 * np.pi * X / scale).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xr = X.copy()
    if disc is not None:
        Xr[np.asarray(disc, bool)] = np.rint(Xr[np.asarray(disc, bool)])
    f_lam, f_amp, f_noise = latent(d)
    ev = lambda f, Z: np.array([f(Z[:, j] / scale) for j in range(Z.shape[1])])            # noqa: E731
    lam0, amp0, noi0 = ev(f_lam, Xr).T, ev(f_amp, Xr), ev(f_noise, X)
    r2 = np.random.default_rng(seed + 50)
    c, a, nz = r2.uniform(0.7, 1.6, S), r2.uniform(0.6, 1.8, S), r2.uniform(1.0, 3.0, S)
    lam = np.asfortranarray(lam0[:, :, None] * c[None, None, :])
    amp = np.asfortranarray(amp0[:, None] * a[None, :])
    noi = np.asfortranarray(noi0[:, None] * nz[None, :])
    return X, y, lam, amp, noi


def ns_oracle(O, X, y, lam, amp, noi, mean=None, disc=None):
    out = []
    for s in range(lam.shape[2]):
        m = None if mean is None else (mean if np.ndim(mean) == 1 else mean[s])
        post = O.nonstationary_fit(X, y, lam[:, :, s], amp[:, s], noi[:, s], mean=m, discrete=disc)
        assert np.isfinite(post.logpdf)
        out.append((post.logpdf, np.linalg.cond(post.L @ post.L.T)))
    return np.array(out).T


def check_parity(ll, st, want, cond, N, what):
    assert ll.shape == want.shape and not st.any(), (what, st)
    for s in range(len(want)):
        err, tol = abs(ll[s] - want[s]), ll_tol(cond[s], N) * (1 + abs(want[s]))
        print(f"[model-batch] {what} set {s}: ll {ll[s]:.12g} oracle {want[s]:.12g} |d| {err:.3e} tol {tol:.3e} cond {cond[s]:.3e}")
        assert err <= tol, (what, s, ll[s], want[s], cond[s])


# ------------------------------------------------------------------------------------------ 1. parity with the oracle
GRAD_SHAPES = [(20, 2, 12, k, False) for k in KERNELS] + [(40, 5, 8, "matern52", False), (113, 8, 6, "matern52", False),
                                                          (43, 2, 6, "matern32", False),      # 129 rows: one past a 128 boundary
                                                          (30, 3, 6, "sqexp", True)]          # two coincident points


@pytest.mark.parametrize("n,d,S,kernel,dup", GRAD_SHAPES)
def test_gradient_batch_parity(api, O, n, d, S, kernel, dup):
    X, y, dY, lam, amp, sig, sgd = grad_case(n, d, S, seed=n + d, dup=dup)
    want, cond = grad_oracle(O, X, y, dY, kernel, lam, amp, sig, sgd)
    ll, st = api.ggp_loglike_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    check_parity(ll, st, want, cond, n * (1 + d), f"ggp n={n} d={d} {kernel}")


@pytest.mark.parametrize("d,N,S", [(2, 50, 12), (8, 300, 12), (3, 1100, 6)])
def test_nonstationary_batch_parity(api, O, d, N, S):
    X, y, lam, amp, noi = ns_case(d, N, S)
    want, cond = ns_oracle(O, X, y, lam, amp, noi)
    ll, st = api.ngp_loglike_batch(X, y, lam, amp, noi)
    check_parity(ll, st, want, cond, N, f"ngp d={d} N={N}")


def test_nonstationary_batch_prior_mean_and_discrete(api, O):
    d, N, S = 3, 200, 5
    X, y, lam, amp, noi = ns_case(d, N, S)
    m_shared = 0.3 * X[0]
    m_per = np.stack([(0.1 + 0.2 * s) * X[1] for s in range(S)])
    for mean, what in ((m_shared, "shared mean"), (m_per, "per-set mean")):
        want, cond = ns_oracle(O, X, y, lam, amp, noi, mean=mean)
        ll, st = api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=mean)
        check_parity(ll, st, want, cond, N, "ngp " + what)
    disc = [False, True, False]
    X, y, lam, amp, noi = ns_case(d, N, S, disc=disc)
    want, cond = ns_oracle(O, X, y, lam, amp, noi, disc=disc)
    ll, st = api.ngp_loglike_batch(X, y, lam, amp, noi, discrete=disc)
    check_parity(ll, st, want, cond, N, "ngp discrete")
    ll_plain, _ = api.ngp_loglike_batch(X, y, lam, amp, noi)
    assert not np.array_equal(ll, ll_plain)                      # the rounding reached the kernel


# ------------------------------------------------------------------------------------------ 2. the single-handle path
@pytest.mark.parametrize("n,d,S,kernel", [(20, 2, 12, "matern52"), (113, 8, 6, "sqexp")])
def test_gradient_batch_agrees_with_single_updates(api, O, n, d, S, kernel):
    """Set s of the batch against boss_ggp_update at the same parameters: within the tolerance, and in every bit — the matrices come
    out of the same kernel, and the batched schedules (look-ahead up to 8 sets, paired panels beyond; both occur among these
    shapes) leave the same factor as a handle's update under the resident chain."""
    X, y, dY, lam, amp, sig, sgd = grad_case(n, d, S, seed=n + d)
    want, cond = grad_oracle(O, X, y, dY, kernel, lam, amp, sig, sgd)
    ll, st = api.ggp_loglike_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    g = api.GradGP(X, y, dY, kernel)
    single = np.array([g.update(lam[:, s], amp[s], sig[s], sgd[s]) for s in range(S)])
    g.close()
    print(f"[model-batch] ggp n={n} d={d}: batch == single bitwise for {int((ll == single).sum())} of {S} sets, max |d| {np.abs(ll - single).max():.3e}")
    for s in range(S):
        assert abs(ll[s] - single[s]) <= ll_tol(cond[s], n * (1 + d)) * (1 + abs(want[s])), (s, ll[s], single[s])
    assert not st.any() and np.array_equal(ll, single)


@pytest.mark.parametrize("d,N,S", [(2, 50, 12), (8, 300, 12)])
def test_nonstationary_batch_agrees_with_single_updates(api, O, d, N, S):
    X, y, lam, amp, noi = ns_case(d, N, S)
    want, cond = ns_oracle(O, X, y, lam, amp, noi)
    ll, st = api.ngp_loglike_batch(X, y, lam, amp, noi)
    g = api.GibbsGP(X, y)
    single = np.array([g.update(lam[:, :, s], amp[:, s], noi[:, s]) for s in range(S)])
    g.close()
    print(f"[model-batch] ngp d={d} N={N}: batch == single bitwise for {int((ll == single).sum())} of {S} sets, max |d| {np.abs(ll - single).max():.3e}")
    for s in range(S):
        assert abs(ll[s] - single[s]) <= ll_tol(cond[s], N) * (1 + abs(want[s])), (s, ll[s], single[s])
    assert not st.any() and np.array_equal(ll, single)


# ------------------------------------------------------------------------------------------ 3. determinism, position, chunks
CHUNK_S = 24                                                     # two chunks of 12: both halves and the whole take the paired batched schedule


def chunk_cases():
    """(name, thunk) of the calls the two-chunk test repeats in a child: 384-row systems, 1.5 MiB per matrix."""
    def ggp(api):
        X, y, dY, lam, amp, sig, sgd = grad_case(128, 2, CHUNK_S, seed=7)
        return api.ggp_loglike_batch(X, y, dY, "matern52", lam, amp, sig, sgd)

    def ngp(api):
        X, y, lam, amp, noi = ns_case(3, 300, CHUNK_S)
        return api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=np.stack([0.1 * s * X[0] for s in range(CHUNK_S)]))
    return {"ggp": ggp, "ngp": ngp}


def poison_cases():
    """One case of each model whose padding rows and columns matter (129 and 300 rows in 256- and 384-row matrices)."""
    def ggp(api):
        X, y, dY, lam, amp, sig, sgd = grad_case(43, 2, 6, seed=45)
        return api.ggp_loglike_batch(X, y, dY, "matern32", lam, amp, sig, sgd)

    def ngp(api):
        X, y, lam, amp, noi = ns_case(8, 300, 12)
        return api.ngp_loglike_batch(X, y, lam, amp, noi)
    return {"ggp": ggp, "ngp": ngp}


def run_child(cases, env_extra, tmp_path):
    out = os.path.join(str(tmp_path), "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), cases, out], env=dict(os.environ, **env_extra), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return np.load(out)


def test_batches_are_deterministic_and_position_independent(api):
    X, y, dY, lam, amp, sig, sgd = grad_case(113, 8, 12, seed=9)
    ll, st = api.ggp_loglike_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
    ll2, _ = api.ggp_loglike_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
    perm = np.random.default_rng(1).permutation(12)
    ll_p, st_p = api.ggp_loglike_batch(X, y, dY, "matern52", lam[:, perm], amp[perm], sig[perm], sgd[perm])
    assert not st.any() and np.array_equal(ll, ll2) and np.array_equal(ll_p, ll[perm]) and np.array_equal(st_p, st[perm])
    X, y, lam, amp, noi = ns_case(8, 300, 12)
    ll, st = api.ngp_loglike_batch(X, y, lam, amp, noi)
    ll2, _ = api.ngp_loglike_batch(X, y, lam, amp, noi)
    ll_p, _ = api.ngp_loglike_batch(X, y, lam[:, :, perm], amp[:, perm], noi[:, perm])
    assert not st.any() and np.array_equal(ll, ll2) and np.array_equal(ll_p, ll[perm])
    # S = 0 is a no-op
    e, es = api.ggp_loglike_batch(X[:2, :5], y[:5], np.zeros((2, 5)), "sqexp", np.zeros((2, 0)), [], [], [])
    assert e.shape == (0,) and es.shape == (0,)
    e, es = api.ngp_loglike_batch(X, y, np.zeros((8, 300, 0)), np.zeros((300, 0)), np.zeros((300, 0)))
    assert e.shape == (0,) and es.shape == (0,)


def test_two_chunks_agree_bitwise_with_one(api, tmp_path):
    """BOSS_MODEL_BATCH_CHUNK_MB=18 (read once per process, so in a child) cuts the 24 matrices of 1.5 MiB into two chunks."""
    child = run_child("chunk", {"BOSS_MODEL_BATCH_CHUNK_MB": "18"}, tmp_path)
    for name, call in chunk_cases().items():
        ll, st = call(api)
        assert not st.any() and np.isfinite(ll).all()
        assert np.array_equal(child[name + "_ll"], ll) and np.array_equal(child[name + "_st"], st), name


# ------------------------------------------------------------------------------------------ 4. failures stay local
def test_gradient_batch_failures_stay_local(api, O):
    """Three coincident points (tests/test_gpu_parity.py, test_gradient_gp_errors_and_unsupported_entry_points): without noise the
    augmented matrix is singular — in the oracle as on the device —, with noise 0.1 it is fine.  Plus sets with a negative parameter."""
    d, n = 2, 12
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (d, n))
    w = np.linspace(1.0, 2.0, d)[:, None]
    y = np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(d)
    dY = 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(d)
    X[:, 1] = X[:, 2] = X[:, 0]
    S = 6
    lam = np.full((d, S), 0.5)
    amp, sig, sgd = np.ones(S), np.full(S, 0.1), np.full(S, 0.1)
    sig[1] = sgd[1] = 0.0                                        # not PD
    lam[1, 2] = -0.1                                             # invalid: negative lengthscale
    sgd[4] = -1.0                                                # invalid: negative gradient noise
    lam[:, 5], amp[5] = [0.7, 0.4], 1.3
    bad_pd, bad_inv = [1], [2, 4]
    for s in range(S):
        if s in bad_inv:
            continue
        if s in bad_pd:
            with pytest.raises(O.PosDefException):
                O.gradient_gp_fit(X, y, dY, "sqexp", lam[:, s], amp[s], sig[s], sgd[s])
        else:
            assert np.isfinite(O.gradient_gp_fit(X, y, dY, "sqexp", lam[:, s], amp[s], sig[s], sgd[s]).logpdf)
    ll, st = api.ggp_loglike_batch(X, y, dY, "sqexp", lam, amp, sig, sgd)
    assert st.tolist() == [0, api.BOSS_E_NOT_PD, api.BOSS_E_INVALID, 0, api.BOSS_E_INVALID, 0], st
    assert all(ll[s] == -np.inf for s in bad_pd + bad_inv)
    good = [0, 3, 5]
    want, cond = grad_oracle(O, X, y, dY, "sqexp", lam[:, good], amp[good], sig[good], sgd[good])
    check_parity(ll[good], st[good], want, cond, n * (1 + d), "ggp beside failed sets")


def test_nonstationary_batch_failures_stay_local(api, O):
    """Identical points (test_nonstationary_gp_discrete_errors_and_host_mirror): zero noise is not PD, noise 0.5 is.  Plus a negative,
    a NaN and an infinite latent value."""
    d = 3
    X0 = np.random.default_rng(4).uniform(0, 1, (d, 1))
    X = np.tile(X0, (1, 4))
    y = np.arange(4.0)
    S = 6
    lam, amp, noi = np.ones((d, 4, S), order="F"), np.ones((4, S), order="F"), np.full((4, S), 0.5, order="F")
    noi[:, 1] = 0.0                                              # not PD
    amp[2, 2] = -1.0
    lam[1, 3, 3] = np.nan
    noi[0, 4] = np.inf
    lam[:, :, 5], amp[:, 5] = 0.6, 1.4
    for s in (0, 5):
        assert np.isfinite(O.nonstationary_fit(X, y, lam[:, :, s], amp[:, s], noi[:, s]).logpdf)
    with pytest.raises(O.PosDefException):
        O.nonstationary_fit(X, y, lam[:, :, 1], amp[:, 1], noi[:, 1])
    ll, st = api.ngp_loglike_batch(X, y, lam, amp, noi)
    assert st.tolist() == [0, api.BOSS_E_NOT_PD, api.BOSS_E_INVALID, api.BOSS_E_INVALID, api.BOSS_E_INVALID, 0], st
    assert all(ll[s] == -np.inf for s in (1, 2, 3, 4))
    good = [0, 5]
    want, cond = ns_oracle(O, X, y, lam[:, :, good], amp[:, good], noi[:, good])
    check_parity(ll[good], st[good], want, cond, 4, "ngp beside failed sets")


# ------------------------------------------------------------------------------------------ 5. through the model layer
def two_output_problem(B):
    rng = np.random.default_rng(31)
    d, n, P = 2, 35, 2
    X = rng.uniform(0, 1, (d, n))
    Y = np.stack([np.sin(3 * X[0]) * np.cos(2 * X[1]), X[0] - X[1] ** 2])
    dY = np.stack([np.stack([3 * np.cos(3 * X[0]) * np.cos(2 * X[1]), -2 * np.sin(3 * X[0]) * np.sin(2 * X[1])]),
                   np.stack([np.ones(n), -2 * X[1]])])                     # P × d × n
    return d, n, P, X, Y, dY, B.GradientData(X, Y, dY)


def test_gradient_model_batch_equals_the_oracle_sum(api, O, monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import gradient_gp
    d, n, P, X, Y, dY, data = two_output_problem(B)
    rng = np.random.default_rng(32)
    S = 6
    prm = [B.HipGradientGPParams(rng.uniform(0.4, 0.8, (d, P)), rng.uniform(0.8, 1.4, P), rng.uniform(0.02, 0.06, P),
                                 rng.uniform(0.05, 0.2, P)) for _ in range(S)]
    model = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P)
    calls = []
    real = api.ggp_loglike_batch
    monkeypatch.setattr(api, "ggp_loglike_batch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert gradient_gp.batched_call_pays(n * (1 + d), S)
    got = model.data_loglike_batch(data, prm)
    assert len(calls) == P                                       # one batched call per output
    oposts = [[O.gradient_gp_fit(X, Y[i], dY[i], "matern52", p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i],
                                 p.grad_noise_std[i]) for i in range(P)] for p in prm]
    assert np.allclose(got, [sum(o.logpdf for o in op) for op in oposts], rtol=1e-9)
    # a set that is not PD in one output is -inf in the sum (three coincident points, no noise)
    Xd = X.copy()
    Xd[:, 1] = Xd[:, 2] = Xd[:, 0]
    bad = B.HipGradientGPParams(np.full((d, P), 0.5), np.ones(P), np.array([0.0, 0.1]), np.array([0.0, 0.1]))
    ok = B.HipGradientGPParams(np.full((d, P), 0.5), np.ones(P), np.full(P, 0.1), np.full(P, 0.1))
    out = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P, kernel="sqexp").data_loglike_batch(
        B.GradientData(Xd, Y, dY), [ok, bad, ok])
    assert np.isfinite(out[0]) and out[1] == -np.inf and out[2] == out[0]


def test_batched_map_over_the_gradient_model_finds_the_oracle_best(api, O):
    import boss_jl_amd as B
    d, n, P, X, Y, dY, data = two_output_problem(B)
    model = B.HipGradientGaussianProcess(lengthscale_priors=[B.MvLogNormal([-0.5] * d, [0.4] * d)] * P,
                                         amplitude_priors=[B.LogNormal(0.0, 0.4)] * P, noise_std_priors=[B.LogNormal(-3.0, 0.3)] * P,
                                         grad_noise_std_priors=[B.LogNormal(-2.0, 0.3)] * P)
    prob = B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])), model, data)
    fit = B.HipBatchedMAP(samples=40, seed=1)
    best = fit.estimate_parameters(prob)
    allp = fit.estimate_parameters(prob, return_all=True)
    prior = model.params_loglike()

    def oracle_post(p):
        try:
            return sum(O.gradient_gp_fit(X, Y[i], dY[i], "matern52", p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i],
                                         p.grad_noise_std[i]).logpdf for i in range(P)) + prior(p)
        except O.PosDefException:
            return -np.inf
    want = np.array([oracle_post(q.params) for q in allp])
    j = int(np.argmax(want))
    assert np.isfinite(want[j]) and len(allp) == 40
    assert np.array_equal(best.params.lengthscales, allp[j].params.lengthscales) and np.array_equal(best.params.amplitudes, allp[j].params.amplitudes)
    assert abs(best.loglike - want[j]) <= 1e-9 * (1 + abs(want[j]))


def test_nonstationary_model_batch_equals_the_single_models(api, O):
    import boss_jl_amd as B
    d, N, P, S = 2, 150, 2, 5
    rng = np.random.default_rng(6)
    X = rng.uniform(0, 3, (d, N))
    Y = np.stack([np.sin(2 * X[0]) + 0.3 * X[1], np.cos(X[0] * X[1])]) + 0.05 * rng.standard_normal((2, N))
    data = B.ExperimentData(X, Y)
    f_lam, f_amp, f_noise = latent(d)
    disc = [False, True]

    def model(c, a, nz, with_mean):
        return B.HipNonstationaryGP(f_lam=[lambda x: c * f_lam(np.asarray(x) / 3)] * P, f_amp=[lambda x: a * f_amp(np.asarray(x) / 3)] * P,
                                    f_noise=[lambda x: nz * f_noise(np.asarray(x) / 3)] * P,
                                    mean=[lambda x: 0.2 * x[0], None] if with_mean else None, discrete=disc)
    models = [model(0.7 + 0.2 * s, 0.6 + 0.25 * s, 1.0 + 0.5 * s, s % 2 == 0) for s in range(S)]
    got = B.nonstationary_data_loglike_batch(models, data)
    single = np.array([m.data_loglike(data) for m in models])
    assert np.isfinite(single).all()
    for s, m in enumerate(models):
        conds = []
        for i in range(P):
            lam, amp, noi, mu, dd = m._latent_at_data(X, i)
            conds.append(np.linalg.cond(O.nonstationary_fit(X, Y[i], lam, amp, noi, mean=mu, discrete=dd).L))
        tol = sum(ll_tol(c * c, N) for c in conds)               # cond(K) = cond(L)²
        assert abs(got[s] - single[s]) <= tol * (1 + abs(single[s])), (s, got[s], single[s])


# ------------------------------------------------------------------------------------------ 6. poisoned memory
def test_poisoned_allocations(api, O, tmp_path):
    """Every new device allocation filled with NaN patterns (BOSS_POISON_ALLOC=1, a fresh process): the identity padding of the
    matrices, the padded points and parameter blocks and the right-hand-side rows must all be WRITTEN by the call."""
    child = run_child("poison", {"BOSS_POISON_ALLOC": "1"}, tmp_path)
    X, y, dY, lam, amp, sig, sgd = grad_case(43, 2, 6, seed=45)
    want, cond = grad_oracle(O, X, y, dY, "matern32", lam, amp, sig, sgd)
    check_parity(child["ggp_ll"], child["ggp_st"], want, cond, 129, "ggp poisoned")
    X, y, lam, amp, noi = ns_case(8, 300, 12)
    want, cond = ns_oracle(O, X, y, lam, amp, noi)
    check_parity(child["ngp_ll"], child["ngp_st"], want, cond, 300, "ngp poisoned")
    for name, call in poison_cases().items():                    # and the same bits as without the poison
        ll, st = call(api)
        assert np.array_equal(ll, child[name + "_ll"]), name


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api as _api
    res = {}
    for _name, _call in {"chunk": chunk_cases, "poison": poison_cases}[sys.argv[1]]().items():
        _ll, _st = _call(_api)
        res[_name + "_ll"], res[_name + "_st"] = _ll, _st
    np.savez(sys.argv[2], **res)
