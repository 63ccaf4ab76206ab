"""Device append (boss_ggp_append: block rows / re-factorisation on the device, the mixed internal row ordering), reserve and
tracked candidates (boss_ggp_track_create, aug_track_append_kernel) of gradient-observation posteriors, and a sequential batch
over them (B.gradient_sequential_batch).  The oracle is O.gradient_gp_fit / O.gradient_gp_mean_and_var on ALL points in the
reference's ordering [y; ∂₁y; …; ∂_d y].

Tolerances: 1e-9·(1+|ℓ|) on the logpdf, 1e-9 on μ and σ² — those of the neighbouring files.  On the data used here
(make_grad, lam = linspace(0.4, 0.6, d), (α, σ, σ_∂) = (1.1, 0.03, 0.07)) the oracle itself moves by at most 4e-13 (ℓ, relative),
9e-12 (μ) and 8e-15 (σ²) when its rows are permuted into the handle's mixed ordering (up to 700 rows, cond(K) <= 1.4e6), so the
ordering does not eat into the bound."""
import numpy as np
import pytest
import scipy.linalg as sla

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
M_CAND = 41
HYP = (1.1, 0.03, 0.07)                                         # α, σ, σ_∂
HYP2 = (0.9, 0.05, 0.1)                                         # the re-update at the end of a case
KERNELS = ["matern32", "matern52", "sqexp"]


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


def obs(X):
    d = X.shape[0]
    w = np.linspace(1.0, 2.0, d)[:, None]
    y = np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(d)
    dY = 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(d)
    return y, dY


def make_grad(d, n, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, n))
    y, dY = obs(X)
    return X, y, dY


def lam_of(d, c=1.0):
    return c * np.linspace(0.4, 0.6, d)


class Data:
    """nt points with values and gradients and M candidates; candidate 3 lies on training point 2."""

    def __init__(self, d, nt, kernel="matern52", M=M_CAND, X=None):
        self.d, self.kernel = d, kernel
        if X is None:
            X = make_grad(d, nt, seed=3 + d)[0]
        self.X = X
        self.y, self.dY = obs(X)
        self.Xs = np.asfortranarray(np.random.default_rng(1000 + d).uniform(0, 1, (d, M)))
        self.Xs[:, 3] = X[:, 2]

    def handle(self, api, n):
        return api.GradGP(self.X[:, :n], self.y[:n], self.dY[:, :n], self.kernel)

    def append(self, g, a, b):
        return g.append(self.X[:, a:b], self.y[a:b], self.dY[:, a:b])

    def oracle(self, O, n, lam=None, hyp=HYP):
        lam = lam_of(self.d) if lam is None else lam
        return O.gradient_gp_fit(self.X[:, :n], self.y[:n], self.dY[:, :n], self.kernel, lam, *hyp)

    def check(self, O, g, lp, n, what, lam=None, hyp=HYP):
        post = self.oracle(O, n, lam, hyp)
        mu, var = g.predict(self.Xs)
        mu_o, var_o = O.gradient_gp_mean_and_var(post, self.Xs)
        e = (abs(lp - post.logpdf) / (1 + abs(post.logpdf)), np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
        print(f"{what} n={n}: logpdf {e[0]:.2e}  mu {e[1]:.2e}  var {e[2]:.2e}", flush=True)
        assert g.n == n and g.N == n * (1 + self.d), (g.n, g.N, n)
        assert e[0] <= 1e-9 and e[1] <= 1e-9 and e[2] <= 1e-9, (what, n, e)
        return post


class Capacity:
    """The handle's storage (rows, a multiple of 256) and from it the path an append must take, in rows = points·(1+d): block rows
    where at most 4 block rows of 128 hold new rows (after a growth: all block rows from the first new row on) and that is not
    the whole matrix."""

    def __init__(self, N):
        self.cap = -(-N // 256) * 256

    def path(self, N0, n):
        N1 = N0 + n
        grown = N1 > self.cap
        if grown:
            self.cap = -(-N1 // 256) * 256
        nblk = self.cap // 128
        rows = (nblk - 1 if grown else (N1 - 1) // 128) - N0 // 128 + 1
        return 1 if rows <= 4 and rows < nblk else 2


def end_of_case(api, O, D, g, n):
    """On the appended (mixed-order) handle: likelihood gradient, candidate gradients and value covariance at the append's
    parameters, then an update with other hyper-parameters — all against fresh oracle fits of all points."""
    d, lam = D.d, lam_of(D.d)
    X, y, dY = D.X[:, :n], D.y[:n], D.dY[:, :n]
    post = D.oracle(O, n)
    # ∂ℓ/∂(λ, α, σ, σ_∂): the bound of tests/test_gpu_parity.py::test_gradient_gp_likelihood_gradient (100 × 1e-9, relative)
    ll_o, gr_o = O.gradient_gp_loglike_grad(X, y, dY, D.kernel, lam, *HYP)
    ll, gr = g.loglike_grad()
    e = (abs(ll - ll_o) / (1 + abs(ll_o)), np.abs(gr - gr_o).max() / (1 + np.abs(gr_o).max()))
    print(f"loglike_grad: ll {e[0]:.2e}  grad {e[1]:.2e}", flush=True)
    assert e[0] <= 1e-9 and e[1] <= 1e-7, e
    # ∇μ, ∇σ²: the bounds of tests/test_gpu_parity.py::test_gradient_gp_candidate_gradients
    K = O.augmented_kernel_matrix(D.kernel, X, lam, *HYP)
    tol = max(1e-9, np.linalg.cond(K) * K.shape[0] * 2.0 ** -53 * 8)
    Xg = np.asfortranarray(D.Xs[:, 4:])                         # (without the candidate on a training point: σ² is clipped there)
    mu_o, var_o, dmu_o, dvar_o = O.gradient_gp_mean_and_var_grad(post, Xg)
    mu, var, dmu, dvar = g.predict_grad(Xg)
    e = (np.abs(mu - mu_o).max(), np.abs(var - np.maximum(var_o, 0)).max(), np.abs(dmu - dmu_o).max() / (1 + np.abs(dmu_o).max()),
         np.abs(dvar - dvar_o).max() / (1 + np.abs(dvar_o).max()))
    print(f"predict_grad: mu {e[0]:.2e} var {e[1]:.2e} dmu {e[2]:.2e} dvar {e[3]:.2e} (tol {tol:.2e})", flush=True)
    assert e[0] <= 1e-9 and e[1] <= 1e-9 and e[2] <= 10 * tol and e[3] <= 10 * tol, (e, tol)
    # value covariance
    Ks = O.augmented_cross_cov(D.kernel, post.X, post.lengthscale, post.amplitude, D.Xs)
    V = sla.solve_triangular(post.L, Ks, lower=True, check_finite=False)
    kid = O.KERNEL_NAMES[D.kernel]
    S_o = (post.amplitude + 1e-8) ** 2 * O.kappa(kid, O.scaled_distance(D.Xs, D.Xs, post.lengthscale + 1e-8)) - V.T @ V
    mu_c, S = g.predict_value_cov(D.Xs)
    e = (np.abs(mu_c - Ks.T @ post.alpha).max(), np.abs(S - S_o).max())
    print(f"cov: mu {e[0]:.2e}  cov {e[1]:.2e}", flush=True)
    assert e[0] <= 1e-9 and e[1] <= 1e-9, e
    # other hyper-parameters on the mixed-order handle
    lam2 = lam_of(d, 1.2)
    lp = g.update(lam2, *HYP2)
    D.check(O, g, lp, n, "update on the appended handle", lam2, HYP2)
    assert api._append_path(g) in (1, 2)                        # (an update does not touch the record of the last append)


def run_append_case(api, O, d, n0, steps, kernel):
    nt = n0 + sum(steps)
    D = Data(d, nt, kernel)
    g = D.handle(api, n0)
    try:
        assert api._append_path(g) == 0
        lp = g.update(lam_of(d), *HYP)
        D.check(O, g, lp, n0, f"d={d} n0={n0} fit")
        cap, n = Capacity(n0 * (1 + d)), n0
        for m in steps:
            want = cap.path(n * (1 + d), m * (1 + d))
            lp = D.append(g, n, n + m)
            n += m
            D.check(O, g, lp, n, f"d={d} n0={n0} +{m}")
            assert api._append_path(g) == want, (n, m, api._append_path(g), want)
        end_of_case(api, O, D, g, n)
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 1: append parity
APPEND_CASES = [(3, 5, [1, 1, 3]), (3, 31, [1]), (3, 32, [1]), (3, 63, [1, 2]), (3, 127, [3]), (3, 10, [60]), (1, 250, [10]),
                (8, 56, [2]), (16, 30, [1, 1])]
CHEAP = {(3, 5), (3, 31), (3, 32), (3, 63)}                     # all three kernels where the case is cheap
APPEND_PARAMS = [(d, n0, st, k) for d, n0, st in APPEND_CASES for k in KERNELS if k == "matern52" or (d, n0) in CHEAP]


@pytest.mark.parametrize("d,n0,steps,kernel", APPEND_PARAMS)
def test_append_parity(api, O, d, n0, steps, kernel):
    """After every step: logpdf, μ, σ² at 41 candidates against a fresh oracle fit of all points, g.n, g.N and the path the append
    took; at the end the likelihood gradient, the candidate gradients, the value covariance and an update with other
    hyper-parameters on the mixed-order handle."""
    run_append_case(api, O, d, n0, steps, kernel)


def test_boundary_straddles_a_kstar_workgroup_and_a_gram_tile(api, O):
    """n0 = 50, d = 3: the head is 200 rows, so the 64×64 Gram tile of rows 192-255 and the 256-row K* workgroup of rows 0-255 hold
    head rows (component-major) and tail rows (point-major) at once."""
    run_append_case(api, O, 3, 50, [20], "matern52")


# ------------------------------------------------------------------------------------------ 2: duplicate points (row / column roles)
@pytest.mark.parametrize("which", ["head", "tail"])
def test_duplicate_points(api, O, which):
    """An appended point equal to a head point / to an earlier appended point: the same-point and duplicate-point entries are the
    ones the reference evaluates at x_j + 1e-8 (gradient_gp.jl:148-152), and there the value × derivative entries depend on which
    observation plays the row.  Wrong roles move μ by 1.6e-8 … 8e-7 on these data, well above the bound."""
    d, n0 = 3, 64
    X = make_grad(d, n0 + 2, seed=11)[0]
    if which == "head":
        X[:, n0 + 1] = X[:, 7]
    else:
        X[:, n0 + 1] = X[:, n0]
    D = Data(d, n0 + 2, X=X)
    g = D.handle(api, n0)
    try:
        g.update(lam_of(d), *HYP)
        lp = D.append(g, n0, n0 + 1)
        D.check(O, g, lp, n0 + 1, f"dup {which}: first")
        lp = D.append(g, n0 + 1, n0 + 2)
        D.check(O, g, lp, n0 + 2, f"dup {which}: the duplicate")
        assert api._append_path(g) == 1
        ll_o, gr_o = O.gradient_gp_loglike_grad(D.X, D.y, D.dY, D.kernel, lam_of(d), *HYP)
        ll, gr = g.loglike_grad()
        assert abs(ll - ll_o) <= 1e-9 * (1 + abs(ll_o)) and np.abs(gr - gr_o).max() <= 1e-7 * (1 + np.abs(gr_o).max())
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 3: behaviour
def test_append_before_the_first_update_raises(api):
    D = Data(3, 12)
    g = D.handle(api, 10)
    try:
        with pytest.raises(api.BossError) as e:
            D.append(g, 10, 11)
        assert e.value.code == api.BOSS_E_NOT_FITTED and g.n == 10 and api._append_path(g) == 0
    finally:
        g.close()


def test_failed_append_reports_what_is_in_the_handle(api, O):
    """Coincident points without noise make the augmented matrix singular (as tests/test_gpu_parity.py builds its failing fits):
    the append fails, the points stay in the handle, and an update with noise serves all of them."""
    d, n0, m = 2, 8, 3
    X = make_grad(d, n0 + m, seed=5)[0]
    X[:, n0:] = X[:, :1]
    D = Data(d, n0 + m, "sqexp", X=X)
    lam = np.array([0.25, 0.3])
    with pytest.raises(O.PosDefException):
        D.oracle(O, n0 + m, lam, (1.0, 0.0, 0.0))
    g = D.handle(api, n0)
    try:
        lp = g.update(lam, 1.0, 0.0, 0.0)
        assert np.isfinite(lp)
        with pytest.raises(api.PosDefException):
            D.append(g, n0, n0 + m)
        assert g.n == n0 + m and g.N == (n0 + m) * (1 + d)
        with pytest.raises(api.BossError) as e:
            g.predict(D.Xs)
        assert e.value.code == api.BOSS_E_NOT_FITTED
        lp = g.update(lam, 1.0, 0.05, 0.1)
        D.check(O, g, lp, n0 + m, "update after the failed append", lam, (1.0, 0.05, 0.1))
    finally:
        g.close()


def test_set_member_leaves_its_set(api, O):
    d, n, S = 3, 40, 3
    D = Data(d, n + 1)
    lam = np.stack([lam_of(d, c) for c in (1.0, 1.1, 1.2)], axis=1)
    amp, sig, sgd = np.array([1.1, 1.0, 0.9]), np.array([0.03, 0.04, 0.05]), np.array([0.07, 0.08, 0.09])
    gps, _, st = api.ggp_fit_batch(D.X[:, :n], D.y[:n], D.dY[:, :n], D.kernel, lam, amp, sig, sgd)
    try:
        assert not st.any()
        before = [g.predict(D.Xs) for g in gps]
        lp = D.append(gps[1], n, n + 1)
        assert api._append_path(gps[1]) == 1
        for s in (0, 2):
            after = gps[s].predict(D.Xs)
            assert np.array_equal(after[0], before[s][0]) and np.array_equal(after[1], before[s][1]), s
            assert gps[s].n == n
            post = D.oracle(O, n, lam[:, s], (amp[s], sig[s], sgd[s]))
            mu_o, var_o = O.gradient_gp_mean_and_var(post, D.Xs)
            assert np.abs(after[0] - mu_o).max() <= 1e-9 and np.abs(after[1] - var_o).max() <= 1e-9
        D.check(O, gps[1], lp, n + 1, "set member", lam[:, 1], (amp[1], sig[1], sgd[1]))
    finally:
        for g in gps:
            g.close()


def test_reserve_then_single_appends(api, O):
    d, n0, m = 3, 62, 6                                         # 248 rows -> 272: without the reserve the third append would grow
    D = Data(d, n0 + m)
    g = D.handle(api, n0)
    try:
        g.update(lam_of(d), *HYP)
        with pytest.raises(api.BossError):                      # the positional form counts observations and stays refused
            g.reserve(n0 + m)
        g.predict(D.Xs)                                         # (still fitted)
        g.reserve(points=n0 + m)
        with pytest.raises(api.BossError) as e:                 # reserve leaves the handle unfitted
            D.append(g, n0, n0 + 1)
        assert e.value.code == api.BOSS_E_NOT_FITTED
        lp = g.update(lam_of(d), *HYP)
        D.check(O, g, lp, n0, "update after reserve")
        cand = api.Candidates(D.Xs)
        tr = api.GradTrack(g, cand)                             # a track's capacity is the handle's: it lasts while nothing grows
        try:
            for j in range(m):
                lp = D.append(g, n0 + j, n0 + j + 1)
                assert api._append_path(g) == 1, j
                post = D.check(O, g, lp, n0 + j + 1, "reserved")
                mu, var = tr.moments()
                mu_o, var_o = O.gradient_gp_mean_and_var(post, D.Xs)
                assert np.abs(mu - mu_o).max() <= 1e-9 and np.abs(var - var_o).max() <= 1e-9, j
        finally:
            tr.close()
            cand.close()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 4: tracks
@pytest.mark.parametrize("d,n0,steps", [(3, 40, [1, 3]), (16, 20, [2])])
def test_tracks(api, O, d, n0, steps):
    """M = 41: two slabs, the second ragged; candidate 3 lies on a training point.  d = 16: two points are 34 rows = 5 launches."""
    nt = n0 + sum(steps)
    D = Data(d, nt)
    g = D.handle(api, n0)
    cand = api.Candidates(D.Xs)
    tr = None
    try:
        g.update(lam_of(d), *HYP)
        tr = api.GradTrack(g, cand)
        coefs, best = [1.0], 0.2
        # EI from moments within 2e-9 of each other: |ΔEI| <= |Δμ| + φ(0) |Δσ| and |Δσ| <= sqrt(|Δσ²|)
        ei_bound = 2e-9 + 0.4 * np.sqrt(2e-9)
        n = n0
        for m in [0] + steps:
            if m:
                D.append(g, n, n + m)
                assert api._append_path(g) == 1
                n += m
            mu, var = tr.moments()
            mu_o, var_o = O.gradient_gp_mean_and_var(D.oracle(O, n), D.Xs)
            mu_p, var_p = g.predict(D.Xs)
            e = (np.abs(mu - mu_o).max(), np.abs(var - var_o).max(), np.abs(mu - mu_p).max(), np.abs(var - var_p).max())
            print(f"track d={d} n={n}: oracle mu {e[0]:.2e} var {e[1]:.2e}  predict mu {e[2]:.2e} var {e[3]:.2e}", flush=True)
            assert max(e) <= 1e-9 and (var >= 0).all(), (n, e)
            acq, am, mx = api.acq_ei_tracks([[tr]], coefs, None, best)
            acq_m, am_m, _ = api.acq_ei_moments(mu[None, None, :], var[None, None, :], coefs, None, best)
            assert np.abs(acq - acq_m).max() <= 1e-12 and am == am_m
            acq_h, am_h, mx_h = api.acq_ei([[g]], cand, coefs, None, best)
            top = np.sort(acq_h)[-2:]
            print(f"        EI: tracks vs handles {np.abs(acq - acq_h).max():.2e}  gap {top[1] - top[0]:.2e}", flush=True)
            assert np.abs(acq - acq_h).max() <= ei_bound and abs(mx - mx_h) <= ei_bound
            assert top[1] - top[0] > 2 * ei_bound and am == am_h
            tr.sync()
            again = tr.moments()
            assert np.array_equal(again[0], mu) and np.array_equal(again[1], var)
        g.update(lam_of(d, 1.2), *HYP2)                         # other hyper-parameters: the track is stale
        with pytest.raises(api.BossError) as e:
            tr.sync()
        assert e.value.code == api.BOSS_E_INVALID and "re-fitted" in str(e.value)
        with pytest.raises(api.BossError):
            tr.moments()
    finally:
        if tr is not None:
            tr.close()
        cand.close()
        g.close()


def test_track_capacity_and_refusals(api):
    d, n0 = 3, 60                                               # 240 rows: the track holds 256 + 256
    D = Data(d, n0 + 70)
    g = D.handle(api, n0)
    cand = api.Candidates(D.Xs)
    plain = api.GP(D.X, D.y, "matern52")
    tr = None
    try:
        with pytest.raises(api.BossError) as e:
            api.GradTrack(g, cand)                              # unfitted
        assert e.value.code == api.BOSS_E_NOT_FITTED
        plain.update(lam_of(d), 1.0, 0.1)
        with pytest.raises(api.BossError) as e:
            api.GradTrack(plain, cand)
        assert e.value.code == api.BOSS_E_INVALID
        g.update(lam_of(d), *HYP)
        with pytest.raises(api.BossError):
            api.Track(g, cand)                                  # the plain model's entry point still refuses these handles
        tr = api.GradTrack(g, cand)
        D.append(g, n0, n0 + 70)                                # 520 rows > 512
        with pytest.raises(api.BossError) as e:
            tr.moments()
        assert e.value.code == api.BOSS_E_INVALID and "capacity" in str(e.value)
    finally:
        if tr is not None:
            tr.close()
        for x in (cand, plain, g):
            x.close()


# ------------------------------------------------------------------------------------------ 5: sequential batch
def test_sequential_batch_equals_the_oracle_loop(api, O, B):
    """P = 2 outputs (EI on output 0 × feasibility of output 1), S = 2 samples, a batch of 3: the tracked loop selects what a host
    loop selects that rebuilds oracle posteriors of all points for every step, with the same speculative observation
    (x, mean_s μ_s(x), mean_s ∇μ_s(x)).  The top two acquisition values of every step differ by more than 1e-6, so no tie decides;
    the acquisition at the selected point agrees with the device's own evaluation to 1e-9."""
    from boss_jl_amd.problem import LinFitness, best_so_far
    d, n, M, S, P, nb = 3, 30, 150, 2, 2, 3
    kernel = "matern52"
    X = make_grad(d, n, seed=12)[0]
    y0, dY0 = obs(X)
    Y = np.stack([y0, 0.5 * np.cos(2 * X[0]) + 0.1 * np.sin(5 * X[1])])
    dY = np.stack([dY0, np.stack([-np.sin(2 * X[0]), 0.5 * np.cos(5 * X[1]), np.zeros(n)])])
    Xs = np.random.default_rng(77).uniform(0, 1, (d, M))
    coefs, y_max = [1.0, 0.0], [np.inf, 0.45]
    prm = [B.HipGradientGPParams(np.stack([lam_of(d, 1.0 + 0.1 * s + 0.05 * i) for i in range(P)], axis=1),
                                 np.array([1.1, 0.8]) + 0.05 * s, np.array([0.03, 0.04]), np.array([0.07, 0.06])) for s in range(S)]
    model = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P, kernel=kernel)
    data = B.GradientData(X.copy(), Y.copy(), dY.copy())
    posts = [[model.model_posterior_slice(p, data, i) for i in range(P)] for p in prm]
    try:
        sel = B.gradient_sequential_batch(posts, Xs, nb, coefs, y_max, Y)
        assert sel.shape == (d, nb)
        Xa, Ya, dYa = X.copy(), Y.copy(), dY.copy()
        for k in range(nb):
            best = best_so_far(LinFitness(coefs), Ya, y_max)
            acq = np.zeros(M)
            ops = [[O.gradient_gp_fit(Xa, Ya[i], dYa[i], kernel, p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i],
                                      p.grad_noise_std[i]) for i in range(P)] for p in prm]
            for row in ops:
                mv = [O.gradient_gp_mean_and_var(po, Xs) for po in row]
                mu, var = np.stack([m[0] for m in mv]), np.stack([m[1] for m in mv])
                acq += O.expected_improvement_lin(coefs, mu, var, best) * O.feas_prob(mu, var, y_max) / S
            am = int(np.argmax(acq))
            top = np.sort(acq)[-2:]
            print(f"step {k}: argmax {am}  max {acq[am]:.6e}  gap {top[1] - top[0]:.2e}", flush=True)
            assert top[1] - top[0] > 1e-6
            x = Xs[:, am]
            assert np.array_equal(sel[:, k], x), (k, am)
            yhat, dyhat = np.zeros(P), np.zeros((P, d))
            for row in ops:
                for i, po in enumerate(row):
                    m_, _, dm_, _ = O.gradient_gp_mean_and_var_grad(po, x[:, None])
                    yhat[i] += m_[0] / S
                    dyhat[i] += dm_[:, 0] / S
            Xa = np.concatenate([Xa, x[:, None]], axis=1)
            Ya = np.concatenate([Ya, yhat[:, None]], axis=1)
            dYa = np.concatenate([dYa, dyhat[:, :, None]], axis=2)
        for s in range(S):                                      # the slices end on the oracle's data, reserved: block rows only
            for i in range(P):
                gp = posts[s][i].gp
                assert gp.n == n + nb and api._append_path(gp) == 1
                po = O.gradient_gp_fit(Xa, Ya[i], dYa[i], kernel, prm[s].lengthscales[:, i], prm[s].amplitudes[i],
                                       prm[s].noise_std[i], prm[s].grad_noise_std[i])
                mu, var = gp.predict(Xs)
                mu_o, var_o = O.gradient_gp_mean_and_var(po, Xs)
                e = (abs(gp.logpdf - po.logpdf) / (1 + abs(po.logpdf)), np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
                print(f"sample {s} output {i}: logpdf {e[0]:.2e} mu {e[1]:.2e} var {e[2]:.2e}", flush=True)
                assert max(e) <= 1e-9, (s, i, e)
    finally:
        for row in posts:
            for p in row:
                p.close()
