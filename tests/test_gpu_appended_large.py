"""Appended model handles of 1024 rows and more (pytest -m gpu).  From there on a prediction leaves the fused path: the
one-launch-per-step substitution with pair updates on the first call, the resident inverse factors from the second few-candidate
call on (few_calls, have_winv), the transposed factor of lt_alloc for the gradients — all of which an append must invalidate or
extend, and for the gradient-observation model all of it over the mixed row ordering.  A re-factorising append (path 2) goes
through the resident chain at this size.  The path every append takes is predicted by the Capacity rule of the single-handle
append tests and asserted (api._append_path).

The reference is the oracle on a fresh fit of ALL points in the reference's own row order.  Tolerances, each from the test that
holds the same quantity to it on fresh handles:
  few-candidate calls (1-3 candidates)           1e-9     tests/test_gpu_parity.py:1420,1433
  first-call steps (M = 150 / 300)               1e-8     tests/test_gpu_parity.py:1450,1461
  logpdf, μ, σ² at 41 candidates, tracks         1e-9     tests/test_gpu_ggp_append_track.py:92,307  tests/test_gpu_ngp_append_track.py:104,288
  gradient model: ∇μ, ∇σ², value covariance, ∂ℓ  tests/test_gpu_ggp_append_track.py:125,135,144 (end_of_case)
  nonstationary: ∇μ, ∇σ²                         tests/test_gpu_parity.py:2066-2073;  ∂ℓ: tests/test_gpu_parity.py:1977-1986
The hyper-parameters of the gradient-observation cases are those of tests/test_gpu_parity.py:1411-1413 (λ = 0.45, α = 1.2, σ = 0.05,
σ_∂ = 0.1), under which that test holds 1200 rows to 1e-9; tests/test_appended_sets_host.py checks that the condition-aware tol of
every case here stays at or below that of the test the bound comes from.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_ggp_append_track as GA      # noqa: E402
import test_gpu_ngp_append_track as NA      # noqa: E402

pytestmark = pytest.mark.gpu
D_ = 3
LAM, HYP = np.full(D_, 0.45), (1.2, 0.05, 0.1)                  # tests/test_gpu_parity.py:1411-1413
LAM2, HYP2 = np.full(D_, 0.5), (1.0, 0.06, 0.12)                # the re-update
GGP_MAIN = (300, [1, 8], 1)                                     # n0, appends, one more under resident inverses: 1200 -> 1240 rows of 1280
GGP_GROWTH = (318, [3], 0)                                      # 1272 -> 1284 rows: the storage grows to 1536
GGP_PATH2 = (260, [140])                                        # 1040 -> 1600 rows, re-factorised
NGP_MAIN = (1100, [1, 5], 1)
NGP_GROWTH = (1275, [10], 0)
NGP_PATH2 = (1030, [600])


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


def few(rng, X, on):
    """the candidates of the few-candidate calls: the first on an appended point, the second on a head point, the rest random"""
    return [X[:, on[0]:on[0] + 1].copy(), X[:, on[1]:on[1] + 1].copy()] + [rng.uniform(0, 1, (X.shape[0], 1)) for _ in range(2)] + \
           [rng.uniform(0, 1, (X.shape[0], 3))]


# ------------------------------------------------------------------------------------------ gradient-observation model
def ggp_predict(O, g, post, Xs, bound, what):
    mu, var = g.predict(Xs)
    mu_o, var_o = O.gradient_gp_mean_and_var(post, Xs)
    e = (np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
    print(f"{what} M={Xs.shape[1]}: mu {e[0]:.2e} var {e[1]:.2e} (<= {bound:.0e})", flush=True)
    assert e[0] <= bound and e[1] <= bound, (what, e)


def ggp_end(O, D, g, n, lam, hyp):
    """predict_grad at 40 candidates, predict_value_cov at 33 and loglike_grad: the bounds of end_of_case"""
    X, y, dY = D.X[:, :n], D.y[:n], D.dY[:, :n]
    post = D.oracle(O, n, lam, hyp)
    ll_o, gr_o = O.gradient_gp_loglike_grad_allpairs(X, y, dY, D.kernel, lam, *hyp)   # (the pair loop takes 20 s at 1240 rows)
    ll, gr = g.loglike_grad()
    e = (abs(ll - ll_o) / (1 + abs(ll_o)), np.abs(gr - gr_o).max() / (1 + np.abs(gr_o).max()))
    print(f"loglike_grad: ll {e[0]:.2e}  grad {e[1]:.2e}", flush=True)
    assert e[0] <= 1e-9 and e[1] <= 1e-7, e
    K = O.augmented_kernel_matrix(D.kernel, X, lam, *hyp)
    tol = max(1e-9, np.linalg.cond(K) * K.shape[0] * 2.0 ** -53 * 8)
    Xg = np.asfortranarray(D.Xs[:, 1:])                         # 40 candidates, the one on a training point among them
    mu_o, var_o, dmu_o, dvar_o = O.gradient_gp_mean_and_var_grad(post, Xg)
    mu, var, dmu, dvar = g.predict_grad(Xg)
    e = (np.abs(mu - mu_o).max(), np.abs(var - np.maximum(var_o, 0)).max(), np.abs(dmu - dmu_o).max() / (1 + np.abs(dmu_o).max()),
         np.abs(dvar - dvar_o).max() / (1 + np.abs(dvar_o).max()))
    print(f"predict_grad: mu {e[0]:.2e} var {e[1]:.2e} dmu {e[2]:.2e} dvar {e[3]:.2e} (tol {tol:.2e})", flush=True)
    assert e[0] <= 1e-9 and e[1] <= 1e-9 and e[2] <= 10 * tol and e[3] <= 10 * tol, (e, tol)
    Xc = np.asfortranarray(D.Xs[:, :33])
    Ks = O.augmented_cross_cov(D.kernel, post.X, post.lengthscale, post.amplitude, Xc)
    V = sla.solve_triangular(post.L, Ks, lower=True, check_finite=False)
    kid = O.KERNEL_NAMES[D.kernel]
    S_o = (post.amplitude + 1e-8) ** 2 * O.kappa(kid, O.scaled_distance(Xc, Xc, post.lengthscale + 1e-8)) - V.T @ V
    mu_c, S = g.predict_value_cov(Xc)
    e = (np.abs(mu_c - Ks.T @ post.alpha).max(), np.abs(S - S_o).max())
    print(f"cov: mu {e[0]:.2e}  cov {e[1]:.2e}", flush=True)
    assert e[0] <= 1e-9 and e[1] <= 1e-9, e


def run_ggp_large(api, O, n0, steps, more, full_end=True):
    """fit, a track of 41 candidates, the appends (block rows, path and logpdf and the track's moments after each), four
    single-candidate calls and one of three candidates (the second of them finds the inverse factors resident), `more` points
    appended under the resident inverses and two more such calls, an update with other hyper-parameters and the M = 150 first
    call; with full_end the gradients, the value covariance and the likelihood gradient."""
    d = D_
    nt = n0 + sum(steps) + more
    D = GA.Data(d, nt)
    rng = np.random.default_rng(n0)
    g = D.handle(api, n0)
    cand = api.Candidates(D.Xs)
    tr = None
    try:
        lp = g.update(LAM, *HYP)
        tr = api.GradTrack(g, cand)
        cap, n = GA.Capacity(n0 * (1 + d)), n0

        def append(m, want_path):
            nonlocal n
            want = cap.path(n * (1 + d), m * (1 + d))
            lp = D.append(g, n, n + m)
            n += m
            post = D.oracle(O, n, LAM, HYP)
            mu, var = tr.moments()
            mu_o, var_o = O.gradient_gp_mean_and_var(post, D.Xs)
            e = (abs(lp - post.logpdf) / (1 + abs(post.logpdf)), np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
            print(f"n0={n0} +{m}: path {api._append_path(g)} logpdf {e[0]:.2e}  track mu {e[1]:.2e} var {e[2]:.2e}", flush=True)
            assert api._append_path(g) == want == want_path, (n, m, api._append_path(g), want)
            assert g.n == n and g.N == n * (1 + d) and max(e) <= 1e-9, (n, e)
            return post
        for m in steps:
            post = append(m, 1)
        for Xs in few(rng, D.X, (n - 1, 5)):
            ggp_predict(O, g, post, Xs, 1e-9, "few")
        if more:
            post = append(more, 1)
            for Xs in (D.X[:, n - 1:n].copy(), rng.uniform(0, 1, (d, 1))):
                ggp_predict(O, g, post, Xs, 1e-9, "few, after an append under resident inverses")
        lp = g.update(LAM2, *HYP2)
        post = D.oracle(O, n, LAM2, HYP2)
        assert abs(lp - post.logpdf) <= 1e-9 * (1 + abs(post.logpdf))
        ggp_predict(O, g, post, np.asfortranarray(rng.uniform(0, 1, (d, 150))), 1e-8, "first call after the update")
        if full_end:
            ggp_end(O, D, g, n, LAM2, HYP2)
    finally:
        if tr is not None:
            tr.close()
        cand.close()
        g.close()


def test_gradient_handle_appended_at_1200_rows(api, O):
    """n0 = 300 (1200 rows of 1280): appends [1, 8] on block rows, the few-candidate calls (1e-9, parity:1420) with the first on an
    appended point and the second on a head point, one more append while the inverse factors are resident, an update with other
    hyper-parameters and M = 150 (1e-8, parity:1450), then ∇μ, ∇σ² at 40 candidates, the value covariance at 33 and ∂ℓ with the
    bounds of end_of_case; a track of 41 candidates follows every append (1e-9)."""
    run_ggp_large(api, O, *GGP_MAIN)


def test_gradient_handle_grows_at_1272_rows(api, O):
    """n0 = 318 (1272 rows) + 3 points = 1284 rows: the storage grows to 1536 and the new rows fill three block rows (path 1 after a
    growth, on arrays ggp_grow_points hands out uninitialised); the track follows through the growth; then the few-candidate and
    M = 150 checks."""
    run_ggp_large(api, O, *GGP_GROWTH, full_end=False)


def run_ggp_path2(api, O):
    n0, steps = GGP_PATH2
    D = GA.Data(D_, n0 + sum(steps))
    g = D.handle(api, n0)
    cand = api.Candidates(D.Xs)
    tr = None
    try:
        g.update(LAM, *HYP)
        tr = api.GradTrack(g, cand)
        want = GA.Capacity(n0 * (1 + D_)).path(n0 * (1 + D_), steps[0] * (1 + D_))
        lp = D.append(g, n0, n0 + steps[0])
        assert api._append_path(g) == want == 2, (api._append_path(g), want)
        D.check(O, g, lp, n0 + steps[0], "re-factorising append", LAM, HYP)
        with pytest.raises(api.BossError) as e:                 # 1600 rows: beyond the track's 1280 + 256
            tr.moments()
        assert e.value.code == api.BOSS_E_INVALID and "capacity" in str(e.value)
    finally:
        if tr is not None:
            tr.close()
        cand.close()
        g.close()


def test_gradient_handle_refactorising_append_at_1040_rows(api, O):
    """n0 = 260 (1040 rows) + 140 points = 1600 rows: six block rows hold new rows, so the append re-factorises (path 2) through the
    resident chain in the mixed ordering; logpdf, μ, σ² at 41 candidates as Data.check holds them (1e-9).  The track created before
    the append holds 1280 + 256 rows and refuses the 1600 (tests/test_gpu_ggp_append_track.py::test_track_capacity_and_refusals)."""
    run_ggp_path2(api, O)


# ------------------------------------------------------------------------------------------ nonstationary model
class BigData(NA.Data):
    """The data of tests/test_gpu_ngp_append_track.py with the noise latent scaled by 1.3: at 1100 and more observations the
    condition-aware tol then stays below that of tests/test_gpu_parity.py::test_nonstationary_gp_candidate_gradients' own data
    (tests/test_appended_sets_host.py)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.noi = 1.3 * self.noi


def ngp_predict(O, D, g, post, Xs, bound, what):
    lamS, ampS, mS = NA.ev(D.fl, Xs).T, NA.ev(D.fa, Xs), (0.3 * Xs[0] if D.mX is not None else None)
    mu, var = g.predict(Xs, lamS, ampS, mS)
    mu_o, var_o = O.nonstationary_mean_and_var(post, Xs, lamS, ampS, mean_s=mS)
    e = (np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
    print(f"{what} M={Xs.shape[1]}: mu {e[0]:.2e} var {e[1]:.2e} (<= {bound:.0e})", flush=True)
    assert e[0] <= bound and e[1] <= bound, (what, e)


def run_ngp_large(api, O, N0, steps, more, full_end=True):
    """the sequence of run_ggp_large on a nonstationary handle with a prior mean: 2-candidate calls, M = 300 after the update"""
    d = D_
    Nt = N0 + sum(steps) + more
    D = BigData(d, Nt, NA.M_CAND, True, False)
    D2 = BigData(d, Nt, NA.M_CAND, True, False, c=1.15)         # other latent values at the same points
    rng = np.random.default_rng(N0)
    g = D.handle(api, N0)
    cand = api.Candidates(D.Xs)
    tr = None
    try:
        D.update(g, N0)
        tr = api.GibbsTrack(g, cand, D.lamS, D.ampS, D.mS)
        cap, N = NA.Capacity(N0), N0

        def append(n):
            nonlocal N
            want = cap.path(N, n)
            lp = D.append(g, N, N + n)
            N += n
            post = D.oracle(O, N)
            mu, var = tr.moments()
            mu_o, var_o = D.oracle_moments(O, post, clip=False)
            e = (abs(lp - post.logpdf) / (1 + abs(post.logpdf)), np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
            print(f"N0={N0} +{n}: path {api._append_path(g)} logpdf {e[0]:.2e}  track mu {e[1]:.2e} var {e[2]:.2e}", flush=True)
            assert api._append_path(g) == want == 1, (N, n, api._append_path(g), want)
            assert g.N == N and max(e) <= 1e-9, (N, e)
            return post
        for n in steps:
            post = append(n)
        calls = [np.hstack([D.X[:, N - 1:N], D.X[:, 5:6]])] + [rng.uniform(0, 1, (d, 2)) for _ in range(3)]
        for Xs in calls:
            ngp_predict(O, D, g, post, np.asfortranarray(Xs), 1e-9, "few")
        if more:
            post = append(more)
            for Xs in (np.hstack([D.X[:, N - 1:N], rng.uniform(0, 1, (d, 1))]), rng.uniform(0, 1, (d, 2))):
                ngp_predict(O, D, g, post, np.asfortranarray(Xs), 1e-9, "few, after an append under resident inverses")
        lp = D2.update(g, N)
        post = D2.oracle(O, N)
        assert abs(lp - post.logpdf) <= 1e-9 * (1 + abs(post.logpdf))
        ngp_predict(O, D2, g, post, np.asfortranarray(rng.uniform(0, 1, (d, 300))), 1e-8, "first call after the update")
        if full_end:
            tol = max(1e-9, np.linalg.cond(post.L @ post.L.T) * N * 2.0 ** -53 * 8)
            Xg = np.asfortranarray(D2.Xs[:, 1:])
            lamS, ampS, mS = D2.lamS[:, 1:], D2.ampS[1:], D2.mS[1:]
            mg = np.zeros((d, Xg.shape[1]))
            mg[0] = 0.3
            o = O.nonstationary_mean_and_var_grad(post, Xg, lamS, ampS, None, None, mS, mg)
            r = g.predict_grad(Xg, lamS, ampS, None, None, mS, mg)
            e = (np.abs(r[0] - o[0]).max(), np.abs(r[1] - np.maximum(o[1], 0.0)).max(), np.abs(r[2] - o[2]).max(), np.abs(r[3] - o[3]).max())
            b = (tol * (1 + np.abs(o[0]).max()), tol * ampS.max() ** 2, 10 * tol * (1 + np.abs(o[2]).max()), 10 * tol * (1 + np.abs(o[3]).max()))
            print("predict_grad: " + "  ".join(f"{x:.2e} (<= {y:.2e})" for x, y in zip(e, b)), flush=True)
            assert all(x <= y for x, y in zip(e, b)), (e, b)
            ll_o, *grads_o = O.nonstationary_loglike_grad(D2.X[:, :N], D2.y[:N], D2.lam[:, :N], D2.amp[:N], D2.noi[:N], mean=D2.m(0, N))
            ll, *grads = g.loglike_grad()
            assert abs(ll - ll_o) <= tol * (1 + abs(ll_o))
            for got, want in zip(grads, grads_o):
                e = np.abs(got - want).max()
                print(f"loglike_grad: {e:.2e} (<= {100 * tol * (1 + np.abs(want).max()):.2e})", flush=True)
                assert got.shape == want.shape and e <= 100 * tol * (1 + np.abs(want).max())
    finally:
        if tr is not None:
            tr.close()
        cand.close()
        g.close()


def test_nonstationary_handle_appended_at_1100_rows(api, O):
    """N0 = 1100: appends of 1 and 5, four 2-candidate calls (1e-9, parity:1433), an append under resident inverses, an update with
    other latent values and M = 300 (1e-8, parity:1461), ∇μ, ∇σ² (parity:2066-2073) and ∂ℓ (parity:1977-1986); a track of 41
    candidates follows every append (1e-9)."""
    run_ngp_large(api, O, *NGP_MAIN)


def test_nonstationary_handle_grows_at_1275_rows(api, O):
    """N0 = 1275 + 10 = 1285 observations: the storage grows from 1280 to 1536, block rows after a growth; the track follows."""
    run_ngp_large(api, O, *NGP_GROWTH, full_end=False)


def run_ngp_path2(api, O):
    N0, steps = NGP_PATH2
    D = BigData(D_, N0 + steps[0], NA.M_CAND, True, False)
    g = D.handle(api, N0)
    cand = api.Candidates(D.Xs)
    tr = None
    try:
        D.update(g, N0)
        tr = api.GibbsTrack(g, cand, D.lamS, D.ampS, D.mS)
        want = NA.Capacity(N0).path(N0, steps[0])
        lp = D.append(g, N0, N0 + steps[0])
        assert api._append_path(g) == want == 2, (api._append_path(g), want)
        D.check(O, g, lp, N0 + steps[0], "re-factorising append")
        with pytest.raises(api.BossError) as e:                 # 1630 observations: beyond the track's 1280 + 256
            tr.moments()
        assert e.value.code == api.BOSS_E_INVALID and "capacity" in str(e.value)
    finally:
        if tr is not None:
            tr.close()
        cand.close()
        g.close()


def test_nonstationary_handle_refactorising_append_at_1030_rows(api, O):
    """N0 = 1030 + 600: six block rows hold new rows, so the append re-factorises (path 2) through the resident chain; the track
    created before it is out of capacity and says so."""
    run_ngp_path2(api, O)


# ------------------------------------------------------------------------------------------ poisoned allocations
CHILD_POISON = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
entry.build()
from boss_jl_amd import api
from oracle import gp_oracle as O
import test_gpu_appended_large as T
T.%(call)s
print("RES ok")
'''


def poisoned(call, timeout):
    code = CHILD_POISON % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "call": call}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BOSS_POISON_ALLOC="1"), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "RES ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_gradient_growth_on_poisoned_allocations(api):
    """The growth case with every fresh device block filled with NaN patterns (BOSS_POISON_ALLOC=1, a child process): gp_grow and
    ggp_grow_points hand out uninitialised arrays on purpose."""
    poisoned("run_ggp_large(api, O, *T.GGP_GROWTH, full_end=False)", 300)


def test_nonstationary_growth_on_poisoned_allocations(api):
    poisoned("run_ngp_large(api, O, *T.NGP_GROWTH, full_end=False)", 300)


# ------------------------------------------------------------------------------------------ call sequences
def test_random_call_sequences_on_model_handles_with_poisoned_allocations():
    """tools/fuzz_models.py — random sequences of update / predict / gradients / covariance / append / reserve / likelihood gradient /
    track / acquisition gradient on one api.GradGP and one api.GibbsGP handle per case, around 128, 256, 1024 and 1280 rows, each
    result checked against a fresh oracle fit — with every new device allocation filled with NaN patterns (BOSS_POISON_ALLOC=1)."""
    env = dict(os.environ, BOSS_POISON_ALLOC="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_models.py"), "12", "6"], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fuzz_models grad: 12 cases passed" in r.stdout and "fuzz_models gibbs: 12 cases passed" in r.stdout, r.stdout[-3000:]
    print(r.stdout[-400:], flush=True)
