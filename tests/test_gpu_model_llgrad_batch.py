"""GPU tests (pytest -m gpu) of the batched likelihood gradients of the gradient-observation and the nonstationary model:
boss_ggp_loglike_grad_batch / boss_ngp_loglike_grad_batch against the CPU oracle's analytic gradients, against update +
loglike_grad on one resident handle (bit for bit), their determinism and position independence, chunks and the ungrouped path,
local failures, the model layer above them, and poisoned memory.

Tolerance: the bars of the single-handle gradient tests (tests/test_gpu_parity.py, test_gradient_gp_likelihood_gradient and
test_nonstationary_gp_likelihood_gradient), with cond(K) computed from the oracle's matrix —
    tol = max(1e-9, cond(K)·rows·2⁻⁵³·8),   |Δℓ| <= tol (1 + |ℓ|),   max|Δg| <= 100 tol (1 + max|g_oracle|).

Run as a script (`python tests/test_gpu_model_llgrad_batch.py <cases> <out.npz>`) the module evaluates one named group of cases in
a fresh process: the chunk, ungrouped and poisoned-allocation tests start it with their environment switch set.
"""
import itertools
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


# ------------------------------------------------------------------------------------------ cases (tests/test_gpu_model_batch.py)
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


def ggp_single(api, X, y, dY, kernel, lam, amp, sig, sgd):
    """update + loglike_grad per set on ONE resident handle: (ll[S], grad[d+3, S])."""
    g = api.GradGP(X, y, dY, kernel)
    S = lam.shape[1]
    ll, gr = np.zeros(S), np.zeros((lam.shape[0] + 3, S))
    for s in range(S):
        g.update(lam[:, s], amp[s], sig[s], sgd[s])
        ll[s], gr[:, s] = g.loglike_grad()
    g.close()
    return ll, gr


def ngp_single(api, X, y, lam, amp, noi, mean=None, disc=None):
    g = api.GibbsGP(X, y, disc)
    d, N, S = lam.shape
    ll, dl, da, dn, dm = np.zeros(S), np.zeros((d, N, S)), np.zeros((N, S)), np.zeros((N, S)), np.zeros((N, S))
    for s in range(S):
        m = None if mean is None else (mean if np.ndim(mean) == 1 else mean[s])
        g.update(lam[:, :, s], amp[:, s], noi[:, s], m)
        ll[s], dl[:, :, s], da[:, s], dn[:, s], dm[:, s] = g.loglike_grad()
    g.close()
    return ll, dl, da, dn, dm


# ------------------------------------------------------------------------------------------ 1. parity with the oracle
GRAD_SHAPES = [(20, 2, 3, k, False) for k in ("matern32", "matern52", "sqexp")] + [
    (43, 2, 3, "matern32", False),                               # 129 rows: one past a tile and a block
    (30, 3, 3, "sqexp", True),                                   # a duplicated point
    (40, 5, 3, "matern52", False),                               # 240 rows
    (57, 8, 2, "matern52", False)]                               # 513 rows: three 256-row steps of the inverse


@pytest.mark.parametrize("n,d,S,kernel,dup", GRAD_SHAPES)
def test_gradient_batch_gradients_match_the_oracle(api, O, n, d, S, kernel, dup):
    X, y, dY, lam, amp, sig, sgd = grad_case(n, d, S, seed=n + d, dup=dup)
    ll, st, gr = api.ggp_loglike_grad_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    assert ll.shape == (S,) and gr.shape == (d + 3, S) and not st.any(), st
    rows = n * (1 + d)
    for s in range(S):
        ll_o, gr_o = O.gradient_gp_loglike_grad(X, y, dY, kernel, lam[:, s], amp[s], sig[s], sgd[s])
        K = O.augmented_kernel_matrix(kernel, X, lam[:, s], amp[s], sig[s], sgd[s])
        tol = grad_tol(np.linalg.cond(K), rows)
        dll, dg = abs(ll[s] - ll_o), np.abs(gr[:, s] - gr_o).max()
        print(f"[llgrad-batch] ggp n={n} d={d} {kernel} set {s}: |dll| {dll:.3e} (bar {tol * (1 + abs(ll_o)):.3e}) max|dg| {dg:.3e} "
              f"(bar {100 * tol * (1 + np.abs(gr_o).max()):.3e}) cond {np.linalg.cond(K):.3e}")
        assert dll <= tol * (1 + abs(ll_o))
        assert dg <= 100 * tol * (1 + np.abs(gr_o).max()), (s, dg, np.abs(gr_o).max())


@pytest.mark.parametrize("d,N,S,extras", [(2, 50, 3, False), (3, 130, 3, True), (8, 300, 3, False), (4, 520, 2, False)])
def test_nonstationary_batch_gradients_match_the_oracle(api, O, d, N, S, extras):
    disc = [False, True, False] if extras else None              # extras: a discrete dimension and a per-set prior mean
    X, y, lam, amp, noi = ns_case(d, N, S, disc=disc)
    mean = np.stack([(0.1 + 0.2 * s) * X[0] for s in range(S)]) if extras else None
    ll, st, dl, da, dn, dm = api.ngp_loglike_grad_batch(X, y, lam, amp, noi, mean_X=mean, discrete=disc)
    assert dl.shape == (d, N, S) and da.shape == dn.shape == dm.shape == (N, S) and not st.any(), st
    for s in range(S):
        m = None if mean is None else mean[s]
        ll_o, dl_o, da_o, dn_o, dm_o = O.nonstationary_loglike_grad(X, y, lam[:, :, s], amp[:, s], noi[:, s], mean=m, discrete=disc)
        post = O.nonstationary_fit(X, y, lam[:, :, s], amp[:, s], noi[:, s], mean=m, discrete=disc)
        cond = np.linalg.cond(post.L @ post.L.T)
        tol = grad_tol(cond, N)
        print(f"[llgrad-batch] ngp d={d} N={N} set {s}: |dll| {abs(ll[s] - ll_o):.3e} (bar {tol * (1 + abs(ll_o)):.3e}) cond {cond:.3e}")
        assert abs(ll[s] - ll_o) <= tol * (1 + abs(ll_o))
        for name, got, want in (("dlam", dl[:, :, s], dl_o), ("damp", da[:, s], da_o), ("dnoise", dn[:, s], dn_o), ("dmean", dm[:, s], dm_o)):
            err, bar = np.abs(got - want).max(), 100 * tol * (1 + np.abs(want).max())
            print(f"[llgrad-batch]     {name}: max|d| {err:.3e} (bar {bar:.3e})")
            assert got.shape == want.shape and err <= bar, (s, name, err, bar)


# ------------------------------------------------------------------------------------------ 2. the single-handle path, bit for bit
@pytest.mark.parametrize("n,d,S,kernel", [(20, 2, 12, "matern52"),      # a group spans the look-ahead → paired-panel switch at 8 sets
                                          (113, 8, 6, "sqexp")])        # 1017 rows
def test_gradient_batch_equals_single_handle_bitwise(api, n, d, S, kernel):
    X, y, dY, lam, amp, sig, sgd = grad_case(n, d, S, seed=n + d)
    ll, st, gr = api.ggp_loglike_grad_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    ll_1, gr_1 = ggp_single(api, X, y, dY, kernel, lam, amp, sig, sgd)
    ll_b, st_b = api.ggp_loglike_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    print(f"[llgrad-batch] ggp n={n} d={d}: max |dll| {np.abs(ll - ll_1).max():.3e} max |dg| {np.abs(gr - gr_1).max():.3e}")
    assert not st.any() and np.isfinite(gr).all() and np.abs(gr).max() > 0
    assert np.array_equal(ll, ll_1) and np.array_equal(gr, gr_1)
    assert np.array_equal(ll, ll_b) and np.array_equal(st, st_b)  # the 128-padded likelihood batch: the same bits


@pytest.mark.parametrize("d,N,S", [(2, 50, 12), (8, 300, 12)])
def test_nonstationary_batch_equals_single_handle_bitwise(api, d, N, S):
    X, y, lam, amp, noi = ns_case(d, N, S)
    mean = 0.3 * X[0]
    ll, st, dl, da, dn, dm = api.ngp_loglike_grad_batch(X, y, lam, amp, noi, mean_X=mean)
    ll_1, dl_1, da_1, dn_1, dm_1 = ngp_single(api, X, y, lam, amp, noi, mean)
    ll_b, st_b = api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=mean)
    print(f"[llgrad-batch] ngp d={d} N={N}: max |dll| {np.abs(ll - ll_1).max():.3e} max |ddlam| {np.abs(dl - dl_1).max():.3e}")
    assert not st.any() and np.abs(dl).max() > 0 and np.abs(dm).max() > 0
    assert np.array_equal(ll, ll_1) and np.array_equal(dl, dl_1) and np.array_equal(da, da_1) and np.array_equal(dn, dn_1)
    assert np.array_equal(dm, dm_1)
    assert np.array_equal(ll, ll_b) and np.array_equal(st, st_b)


# ------------------------------------------------------------------------------------------ 3. determinism, position
def test_gradient_batches_are_deterministic_and_position_independent(api):
    S = 6
    perm = np.random.default_rng(1).permutation(S)
    X, y, dY, lam, amp, sig, sgd = grad_case(43, 2, S, seed=9)
    a = api.ggp_loglike_grad_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
    b = api.ggp_loglike_grad_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
    p = api.ggp_loglike_grad_batch(X, y, dY, "matern52", lam[:, perm], amp[perm], sig[perm], sgd[perm])
    one = api.ggp_loglike_grad_batch(X, y, dY, "matern52", lam[:, 4:5], amp[4:5], sig[4:5], sgd[4:5])
    assert not a[1].any() and all(np.array_equal(u, v) for u, v in zip(a, b))
    assert np.array_equal(p[0], a[0][perm]) and np.array_equal(p[2], a[2][:, perm])
    assert one[0][0] == a[0][4] and np.array_equal(one[2][:, 0], a[2][:, 4])
    X, y, lam, amp, noi = ns_case(3, 130, S)
    a = api.ngp_loglike_grad_batch(X, y, lam, amp, noi)
    b = api.ngp_loglike_grad_batch(X, y, lam, amp, noi)
    p = api.ngp_loglike_grad_batch(X, y, lam[:, :, perm], amp[:, perm], noi[:, perm])
    one = api.ngp_loglike_grad_batch(X, y, lam[:, :, 4:5], amp[:, 4:5], noi[:, 4:5])
    assert not a[1].any() and all(np.array_equal(u, v) for u, v in zip(a, b))
    assert np.array_equal(p[0], a[0][perm]) and all(np.array_equal(p[k], a[k][..., perm]) for k in (2, 3, 4, 5))
    assert one[0][0] == a[0][4] and all(np.array_equal(one[k][..., 0], a[k][..., 4]) for k in (2, 3, 4, 5))
    # S = 0 is a no-op
    e = api.ggp_loglike_grad_batch(X[:2, :5], y[:5], np.zeros((2, 5)), "sqexp", np.zeros((2, 0)), [], [], [])
    assert e[0].shape == (0,) and e[2].shape == (5, 0)
    e = api.ngp_loglike_grad_batch(X, y, np.zeros((3, 130, 0)), np.zeros((130, 0)), np.zeros((130, 0)))
    assert e[0].shape == (0,) and e[2].shape == (3, 130, 0) and e[5].shape == (130, 0)


# ------------------------------------------------------------------------------------------ 4. chunks, the ungrouped path, poison
CHUNK_S = 24                                                     # two chunks of 12


def child_cases():
    """name -> thunk of the calls the child-process tests repeat.  300-row systems: 512 padded rows, 2.5 MiB per matrix."""
    def ggp(api):
        X, y, dY, lam, amp, sig, sgd = grad_case(100, 2, CHUNK_S, seed=7)
        return api.ggp_loglike_grad_batch(X, y, dY, "matern52", lam, amp, sig, sgd)

    def ngp(api):
        X, y, lam, amp, noi = ns_case(3, 300, CHUNK_S)
        return api.ngp_loglike_grad_batch(X, y, lam, amp, noi, mean_X=np.stack([0.1 * s * X[0] for s in range(CHUNK_S)]))

    def ggp_small(api):                                          # 129 rows in a 256-row matrix: the padding matters
        X, y, dY, lam, amp, sig, sgd = grad_case(43, 2, 6, seed=45)
        return api.ggp_loglike_grad_batch(X, y, dY, "matern32", lam, amp, sig, sgd)

    def ngp_small(api):
        X, y, lam, amp, noi = ns_case(8, 300, 6)
        return api.ngp_loglike_grad_batch(X, y, lam, amp, noi)
    return {"ggp": ggp, "ngp": ngp, "ggp_small": ggp_small, "ngp_small": ngp_small}


GROUPS = {"chunk": ("ggp", "ngp"), "ungrouped": ("ggp", "ngp"), "poison": ("ggp_small", "ngp_small")}


def run_child(group, env_extra, tmp_path):
    out = os.path.join(str(tmp_path), "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), group, out], env=dict(os.environ, **env_extra), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return np.load(out)


def assert_child_equal(api, child, names):
    for name in names:
        res = child_cases()[name](api)
        assert not res[1].any() and np.isfinite(res[0]).all(), name
        for k, arr in enumerate(res):
            assert np.array_equal(child[f"{name}_{k}"], arr), (name, k)


def test_two_chunks_agree_bitwise_with_one(api, tmp_path):
    """BOSS_MODEL_BATCH_CHUNK_MB=30 (read once per process, so in a child) cuts the 24 matrices of 2.5 MiB into two chunks."""
    assert_child_equal(api, run_child("chunk", {"BOSS_MODEL_BATCH_CHUNK_MB": "30"}, tmp_path), GROUPS["chunk"])


def test_ungrouped_path_agrees_bitwise_with_groups(api, tmp_path):
    """BOSS_LLGRAD_GROUP_NP=256 (read once per process): the 512-row sets go set after set over the banks of workspaces."""
    assert_child_equal(api, run_child("ungrouped", {"BOSS_LLGRAD_GROUP_NP": "256"}, tmp_path), GROUPS["ungrouped"])


def test_poisoned_allocations(api, tmp_path):
    """Every new device allocation filled with NaN patterns (BOSS_POISON_ALLOC=1, a fresh process): what the gradient pass reads
    of the padded matrices, parameter blocks and work buffers must all have been WRITTEN by the call."""
    assert_child_equal(api, run_child("poison", {"BOSS_POISON_ALLOC": "1"}, tmp_path), GROUPS["poison"])


# ------------------------------------------------------------------------------------------ 5. failures stay local
def test_gradient_batch_failures_stay_local(api):
    """Three coincident points without noise: the augmented matrix is singular and fails at the pivot check (the construction of
    tests/test_gpu_model_batch.py, test_gradient_batch_failures_stay_local).  Plus a set with a negative parameter."""
    d, n = 2, 12
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 1, (d, n))
    w = np.linspace(1.0, 2.0, d)[:, None]
    y = np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(d)
    dY = 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(d)
    X[:, 1] = X[:, 2] = X[:, 0]
    S = 5
    lam = np.full((d, S), 0.5)
    amp, sig, sgd = np.ones(S), np.full(S, 0.1), np.full(S, 0.1)
    sig[1] = sgd[1] = 0.0                                        # not PD
    lam[1, 2] = -0.1                                             # invalid
    lam[:, 4], amp[4] = [0.7, 0.4], 1.3
    ll, st, gr = api.ggp_loglike_grad_batch(X, y, dY, "sqexp", lam, amp, sig, sgd)
    assert st.tolist() == [0, api.BOSS_E_NOT_PD, api.BOSS_E_INVALID, 0, 0], st
    assert ll[1] == -np.inf and ll[2] == -np.inf and not gr[:, 1].any() and not gr[:, 2].any()
    good = [0, 3, 4]
    ll_g, st_g, gr_g = api.ggp_loglike_grad_batch(X, y, dY, "sqexp", lam[:, good], amp[good], sig[good], sgd[good])
    assert not st_g.any() and np.array_equal(ll[good], ll_g) and np.array_equal(gr[:, good], gr_g) and np.isfinite(gr_g).all()
    # a NULL grad_out is refused
    lib = api.load_library()
    import ctypes as C
    Xf, yf, dYf, lamf = (np.asfortranarray(a, dtype=np.float64) for a in (X, y, dY, lam))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))       # noqa: E731
    rc = lib.boss_ggp_loglike_grad_batch(0, 2, d, n, dp(Xf), dp(yf), dp(dYf), S, dp(lamf), dp(amp), dp(sig), dp(sgd), dp(ll), None,
                                         st.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == api.BOSS_E_INVALID


def test_nonstationary_batch_failures_stay_local_and_null_outputs(api):
    """Identical points with zero noise are not PD (tests/test_gpu_model_batch.py); plus a negative latent value."""
    d = 3
    X0 = np.random.default_rng(4).uniform(0, 1, (d, 1))
    X = np.tile(X0, (1, 4))
    y = np.arange(4.0)
    S = 5
    lam, amp, noi = np.ones((d, 4, S), order="F"), np.ones((4, S), order="F"), np.full((4, S), 0.5, order="F")
    noi[:, 1] = 0.0                                              # not PD
    amp[2, 2] = -1.0                                             # invalid
    lam[:, :, 4], amp[:, 4] = 0.6, 1.4
    res = api.ngp_loglike_grad_batch(X, y, lam, amp, noi)
    ll, st = res[0], res[1]
    assert st.tolist() == [0, api.BOSS_E_NOT_PD, api.BOSS_E_INVALID, 0, 0], st
    assert ll[1] == -np.inf and ll[2] == -np.inf and all(not a[..., 1].any() and not a[..., 2].any() for a in res[2:])
    good = [0, 3, 4]
    res_g = api.ngp_loglike_grad_batch(X, y, lam[:, :, good], amp[:, good], noi[:, good])
    assert not res_g[1].any() and np.array_equal(ll[good], res_g[0])
    assert all(np.array_equal(a[..., good], b) and np.isfinite(b).all() for a, b in zip(res[2:], res_g[2:]))
    # every combination of NULL outputs
    lib = api.load_library()
    import ctypes as C
    Xf = np.asfortranarray(X)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    for mask in itertools.product((False, True), repeat=4):
        outs = [np.full(sh, 7.0, order="F") if m else None for m, sh in zip(mask, ((d, 4, S), (4, S), (4, S), (4, S)))]
        ll2, st2 = np.zeros(S), np.zeros(S, dtype=np.int32)
        rc = lib.boss_ngp_loglike_grad_batch(0, d, 4, dp(Xf), dp(y), None, S, dp(lam), dp(amp), dp(noi), None, 0, dp(ll2), *map(dp, outs),
                                             st2.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == 0 and np.array_equal(ll2, ll) and np.array_equal(st2, st), mask
        for got, want in zip(outs, res[2:]):
            assert got is None or np.array_equal(got, want), mask


# ------------------------------------------------------------------------------------------ 6. through the model layer
def test_gradient_map_is_the_same_through_the_batch_and_the_loop(api, monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import gradient_gp
    rng = np.random.default_rng(31)
    d, n, P = 2, 20, 2
    X = rng.uniform(0, 1, (d, n))
    Y = np.stack([np.sin(3 * X[0]) * np.cos(2 * X[1]), X[0] - X[1] ** 2])
    dY = np.stack([np.stack([3 * np.cos(3 * X[0]) * np.cos(2 * X[1]), -2 * np.sin(3 * X[0]) * np.sin(2 * X[1])]),
                   np.stack([np.ones(n), -2 * X[1]])])
    model = B.HipGradientGaussianProcess(lengthscale_priors=[B.MvLogNormal([-0.5] * d, [0.4] * d)] * P,
                                         amplitude_priors=[B.LogNormal(0.0, 0.4)] * P, noise_std_priors=[B.LogNormal(-3.0, 0.3)] * P,
                                         grad_noise_std_priors=[B.LogNormal(-2.0, 0.3)] * P)
    prob = B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])), model,
                         B.GradientData(X, Y, dY))
    calls = []
    real = api.ggp_loglike_grad_batch
    monkeypatch.setattr(api, "ggp_loglike_grad_batch", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(gradient_gp, "batched_grad_call_pays", lambda rows, S: True)
    via_batch = B.HipGradientMAP(multistart=4, iters=5, seed=11).estimate_parameters(prob)
    assert calls and len(calls) % P == 0
    n_batch = len(calls)
    monkeypatch.setattr(gradient_gp, "batched_grad_call_pays", lambda rows, S: False)
    via_loop = B.HipGradientMAP(multistart=4, iters=5, seed=11).estimate_parameters(prob)
    assert len(calls) == n_batch                                 # the loop made no batched call
    assert np.isfinite(via_batch.loglike) and via_batch.loglike == via_loop.loglike
    for name in ("lengthscales", "amplitudes", "noise_std", "grad_noise_std"):
        assert np.array_equal(getattr(via_batch.params, name), getattr(via_loop.params, name)), name


def test_nonstationary_model_grad_batch_equals_the_single_models(api):
    import boss_jl_amd as B
    d, N, P, S = 2, 150, 2, 3
    rng = np.random.default_rng(6)
    X = rng.uniform(0, 3, (d, N))
    Y = np.stack([np.sin(2 * X[0]) + 0.3 * X[1], np.cos(X[0] * X[1])]) + 0.05 * rng.standard_normal((2, N))
    data = B.ExperimentData(X, Y)
    f_lam, f_amp, f_noise = latent(d)

    def model(c, a, nz, with_mean):
        return B.HipNonstationaryGP(f_lam=[lambda x: c * f_lam(np.asarray(x) / 3)] * P, f_amp=[lambda x: a * f_amp(np.asarray(x) / 3)] * P,
                                    f_noise=[lambda x: nz * f_noise(np.asarray(x) / 3)] * P,
                                    mean=[lambda x: 0.2 * x[0], None] if with_mean else None, discrete=[False, True])
    models = [model(0.7 + 0.2 * s, 0.6 + 0.25 * s, 1.0 + 0.5 * s, s % 2 == 0) for s in range(S)]
    tot, grads = B.nonstationary_data_loglike_grad_batch(models, data)
    assert tot.shape == (S,) and np.isfinite(tot).all()
    for s, m in enumerate(models):
        want = 0.0
        for i, sl in enumerate(m.model_posterior(data)):
            res = sl.loglike_grad()
            sl.close()
            want += res[0]
            for got, w in zip(grads[s][i], res[1:]):
                assert np.array_equal(got, w), (s, i)
        assert tot[s] == want


if __name__ == "__main__":
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api as _api
    out = {}
    for _name in GROUPS[sys.argv[1]]:
        for _k, _arr in enumerate(child_cases()[_name](_api)):
            out[f"{_name}_{_k}"] = _arr
    np.savez(sys.argv[2], **out)
