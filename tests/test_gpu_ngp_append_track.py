"""Device append (boss_ngp_append: block rows / re-factorisation on the device), reserve and tracked candidates
(boss_ngp_track_create[_lat], gibbs_track_append_kernel) of nonstationary posteriors, and SequentialBatchAM over them
(B.nonstationary_sequential_batch).  The oracle is O.nonstationary_fit / O.nonstationary_mean_and_var on ALL points with the
latent closures evaluated at every point.

Tolerances: 1e-9·(1+|ℓ|) on the logpdf, 1e-9 on μ and σ² — those of tests/test_gpu_parity.py::test_nonstationary_gp_append.  On the
data used here (latent() below, σ(x) >= 0.1) the oracle itself moves by at most 2e-13 (logpdf, relative) and 4e-13 (μ, σ²) when the
old points are permuted (cond(K) <= 8e4 at N = 856), so the conditioning of the chosen latents does not eat into the bound."""
import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
M_CAND = 41


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


def make(d, N, M, seed=1, noise=0.05):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + noise * rng.standard_normal(N)
    Xs = np.random.default_rng(seed + 1000).uniform(0, 1, (d, M))
    return X, y, Xs


def latent(d, c=1.0):
    f_lam = lambda x: c * (0.25 + 0.5 * np.asarray(x) ** 2 + 0.1 * np.arange(1, d + 1) / max(1.0, d / 3))   # noqa: E731
    f_amp = lambda x: 1.0 + 0.4 * np.sin(3 * x[0]) / c                                                       # noqa: E731
    f_noise = lambda x: 0.1 + 0.05 * x[-1] ** 2                                                              # noqa: E731
    return f_lam, f_amp, f_noise


def ev(f, Z):
    return np.array([f(Z[:, j]) for j in range(Z.shape[1])])


class Data:
    """Ntot points and M candidates with the latent closures evaluated at all of them (rounded where discrete)."""

    def __init__(self, d, Ntot, M, mean, disc, seed=21, c=1.0):
        self.d = d
        self.X, self.y, self.Xs = make(d, Ntot, M, seed=seed + d)
        self.discrete = None
        if disc:
            self.discrete = np.zeros(d, bool)
            self.discrete[1] = True
            self.X[1] *= 5
            self.Xs[1] *= 5
        self.fl, self.fa, self.fn = latent(d, c)
        self.lam, self.amp, self.noi = ev(self.fl, self.rnd(self.X)).T, ev(self.fa, self.rnd(self.X)), ev(self.fn, self.X)
        self.lamS, self.ampS = ev(self.fl, self.rnd(self.Xs)).T, ev(self.fa, self.rnd(self.Xs))
        self.mX = 0.3 * self.X[0] if mean else None
        self.mS = 0.3 * self.Xs[0] if mean else None

    def rnd(self, Z):
        return Z if self.discrete is None else np.where(self.discrete[:, None], np.rint(Z), Z)

    def m(self, a, b):
        return None if self.mX is None else self.mX[a:b]

    def handle(self, api, N):
        return api.GibbsGP(self.X[:, :N], self.y[:N], self.discrete)

    def update(self, g, N):
        return g.update(self.lam[:, :N], self.amp[:N], self.noi[:N], self.m(0, N))

    def append(self, g, a, b):
        return g.append(self.X[:, a:b], self.y[a:b], self.lam[:, a:b], self.amp[a:b], self.noi[a:b], self.m(a, b))

    def oracle(self, O, N):
        return O.nonstationary_fit(self.X[:, :N], self.y[:N], self.lam[:, :N], self.amp[:N], self.noi[:N], mean=self.m(0, N),
                                   discrete=self.discrete)

    def oracle_moments(self, O, post, clip=True):
        return O.nonstationary_mean_and_var(post, self.Xs, self.lamS, self.ampS, mean_s=self.mS, clip=clip)

    def check(self, O, g, lp, N, what):
        post = self.oracle(O, N)
        mu, var = g.predict(self.Xs, self.lamS, self.ampS, self.mS)
        mu_o, var_o = self.oracle_moments(O, post)
        e = (abs(lp - post.logpdf) / (1 + abs(post.logpdf)), np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
        print(f"{what} N={N}: logpdf {e[0]:.2e}  mu {e[1]:.2e}  var {e[2]:.2e}", flush=True)
        assert g.N == N and e[0] <= 1e-9 and e[1] <= 1e-9 and e[2] <= 1e-9, (what, N, e)
        return post


class Capacity:
    """The handle's storage (rows, a multiple of 256) and from it the path an append must take: block rows where at most 4 block
    rows of 128 hold new rows (after a growth: all block rows from the first new row on) and that is not the whole matrix."""

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


APPEND_CASES = [(3, 5, [1, 1, 3]), (3, 127, [2]), (3, 128, [1]), (3, 255, [1, 130]), (3, 250, [7, 300]), (3, 256, [600]),
                (16, 130, [1, 1]), (17, 130, [1, 1])]
APPEND_PARAMS = [(d, N0, st, mean, False) for d, N0, st in APPEND_CASES for mean in (False, True)] + \
                [(d, N0, st, True, True) for d, N0, st in APPEND_CASES if d == 3]


# ------------------------------------------------------------------------------------------ 1: append parity
@pytest.mark.parametrize("d,N0,steps,mean,disc", APPEND_PARAMS)
def test_append_parity(api, O, d, N0, steps, mean, disc):
    """After every step: logpdf, μ, σ² at 41 candidates against a fresh oracle fit of all points, and the path the append took; at
    the end the factor against the oracle's (1e-10) and a full update with other latents against a fresh oracle fit."""
    Nt = N0 + sum(steps)
    D = Data(d, Nt, M_CAND, mean, disc)
    g = D.handle(api, N0)
    try:
        assert api._append_path(g) == 0
        D.update(g, N0)
        cap, N = Capacity(N0), N0
        for n in steps:
            want = cap.path(N, n)
            lp = D.append(g, N, N + n)
            N += n
            post = D.check(O, g, lp, N, f"d={d} N0={N0} +{n}")
            assert api._append_path(g) == want, (N, n, api._append_path(g), want)
        L, z = g.factor()
        eL = np.abs(L - post.L).max()
        print(f"factor {eL:.2e}", flush=True)
        assert eL <= 1e-10
        D2 = Data(d, Nt, M_CAND, mean, disc, c=1.15)            # other latent values at the same points
        lp = D2.update(g, Nt)
        D2.check(O, g, lp, Nt, "update on the grown handle")
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 2: the old blocks are untouched
def test_block_row_leaves_old_blocks_bit_identical(api):
    D = Data(3, 301, M_CAND, True, False)
    g = D.handle(api, 300)
    try:
        D.update(g, 300)
        L0, _ = g.factor()
        D.append(g, 300, 301)
        assert api._append_path(g) == 1
        L1, _ = g.factor()
        assert np.array_equal(L1[:256, :256], L0[:256, :256])
        assert L1.shape == (301, 301) and np.all(np.isfinite(L1))
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 3: errors
def test_errors(api, O):
    D = Data(3, 160, M_CAND, True, False)
    N = 150
    g = D.handle(api, N)
    try:
        with pytest.raises(api.BossError) as e:
            D.append(g, N, N + 1)                               # before the first update
        assert e.value.code == api.BOSS_E_NOT_FITTED
        D.update(g, N)
        with pytest.raises(api.BossError) as e:
            g.append(D.X[:, N:N + 1], D.y[N:N + 1], D.lam[:, N:N + 1], D.amp[N:N + 1], D.noi[N:N + 1])   # the posterior has a prior mean
        assert e.value.code == api.BOSS_E_INVALID
        ref = g.predict(D.Xs, D.lamS, D.ampS, D.mS)
        sl = slice(N, N + 2)
        for what, lam, amp, noi in (("lam", 0.0, None, None), ("amp", None, -1.0, None), ("noise", None, None, np.nan)):
            l, a, s = D.lam[:, sl].copy(), D.amp[sl].copy(), D.noi[sl].copy()
            if lam is not None:
                l[1, 1] = lam
            if amp is not None:
                a[1] = amp
            if noi is not None:
                s[1] = noi
            with pytest.raises(api.BossError) as e:
                g.append(D.X[:, sl], D.y[sl], l, a, s, D.mX[sl])
            assert e.value.code == api.BOSS_E_INVALID, what
            assert g.N == N and api._append_path(g) == 0
            again = g.predict(D.Xs, D.lamS, D.ampS, D.mS)
            assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1]), what
        # the plain model's entry points still refuse these handles
        with pytest.raises(api.BossError):
            api.GP.append(g, D.X[:, N:N + 1], D.y[N:N + 1])
        with pytest.raises(api.BossError):
            api.GP.reserve(g, N + 10)
        cand = api.Candidates(D.Xs)
        with pytest.raises(api.BossError):
            api.Track(g, cand)
        cand.close()
        again = g.predict(D.Xs, D.lamS, D.ampS, D.mS)
        assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 4: reserve
def test_reserve_then_single_appends(api, O):
    N0, n = 250, 12
    D = Data(3, N0 + n, M_CAND, True, False)
    g = D.handle(api, N0)
    try:
        D.update(g, N0)
        g.reserve(N0 + n)
        with pytest.raises(api.BossError):                      # reserve leaves the handle unfitted
            D.append(g, N0, N0 + 1)
        lp = D.update(g, N0)                                    # latent arrays of N columns, as before
        D.check(O, g, lp, N0, "update after reserve")
        for j in range(n):
            lp = D.append(g, N0 + j, N0 + j + 1)
            assert api._append_path(g) == 1, j
            D.check(O, g, lp, N0 + j + 1, "reserved")
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 5: members of a fitted set
def test_set_member_leaves_its_set(api, O):
    S, N = 3, 140
    Ds = [Data(3, N + 1, M_CAND, True, False, c=c) for c in (1.0, 1.1, 1.2)]
    D0 = Ds[0]
    lam = np.stack([D.lam[:, :N] for D in Ds], axis=2)
    amp = np.stack([D.amp[:N] for D in Ds], axis=1)
    noi = np.stack([D.noi[:N] for D in Ds], axis=1)
    mX = np.stack([D.mX[:N] for D in Ds])
    gps, _, st = api.ngp_fit_batch(D0.X[:, :N], D0.y[:N], lam, amp, noi, mX, None)
    try:
        assert np.all(st == api.BOSS_OK)
        before = [g.predict(D.Xs, D.lamS, D.ampS, D.mS) for g, D in zip(gps, Ds)]
        lp = Ds[1].append(gps[1], N, N + 1)
        assert api._append_path(gps[1]) == 1
        for s in (0, 2):
            after = gps[s].predict(Ds[s].Xs, Ds[s].lamS, Ds[s].ampS, Ds[s].mS)
            assert np.array_equal(after[0], before[s][0]) and np.array_equal(after[1], before[s][1]), s
            assert gps[s].N == N
        Ds[1].check(O, gps[1], lp, N + 1, "set member")
    finally:
        for g in gps:
            g.close()


# ------------------------------------------------------------------------------------------ 6: tracks
@pytest.mark.parametrize("d,N0,steps,mean,disc", [(3, 100, [1, 1, 1], True, False), (3, 250, [3, 9, 1], False, True),
                                                  (16, 120, [8, 9], False, False)])
def test_tracks(api, O, d, N0, steps, mean, disc):
    M = 77                                                      # three slabs, the last ragged
    Nt = N0 + sum(steps)
    D = Data(d, Nt, M, mean, disc)
    g = D.handle(api, N0)
    cand = api.Candidates(D.Xs)
    tr = None
    try:
        D.update(g, N0)
        tr = api.GibbsTrack(g, cand, D.lamS, D.ampS, D.mS)
        coefs, y_max, best = [1.0], [0.4], 0.2
        N = N0
        for n in [0] + steps:
            if n:
                D.append(g, N, N + n)
                N += n
            mu, var = tr.moments()
            mu_o, var_o = D.oracle_moments(O, D.oracle(O, N), clip=False)
            e = (np.abs(mu - mu_o).max(), np.abs(var - var_o).max())
            print(f"track d={d} N={N}: mu {e[0]:.2e}  var {e[1]:.2e}", flush=True)
            assert e[0] <= 1e-9 and e[1] <= 1e-9, (N, e)
            acq, am, mx = api.acq_ei_tracks([[tr]], coefs, y_max, best)
            acq_m, am_m, mx_m = api.acq_ei_moments(mu[None, None, :], var[None, None, :], coefs, y_max, best)
            assert np.abs(acq - acq_m).max() <= 1e-12 and am == am_m
            tr.sync()
            again = tr.moments()
            tr.sync()
            again2 = tr.moments()
            assert np.array_equal(again[0], mu) and np.array_equal(again[1], var)
            assert np.array_equal(again2[0], mu) and np.array_equal(again2[1], var)
        D2 = Data(d, Nt, M, mean, disc, c=1.15)
        D2.update(g, Nt)                                        # other latents: the track is stale
        with pytest.raises(api.BossError) as e:
            tr.sync()
        assert e.value.code == api.BOSS_E_INVALID
        with pytest.raises(api.BossError):
            tr.moments()
    finally:
        if tr is not None:
            tr.close()
        cand.close()
        g.close()


def test_track_create_refusals(api):
    D = Data(3, 60, 77, False, False)
    cand = api.Candidates(D.Xs)
    plain = api.GP(D.X, D.y, "matern52")
    plain.update(np.full(3, 0.5), 1.0, 0.1)
    grad = api.GradGP(D.X[:, :20], D.y[:20], np.zeros((3, 20)), "sqexp")
    grad.update(np.full(3, 0.5), 1.0, 0.1, 0.1)
    g = D.handle(api, 60)
    other = api.Candidates(np.vstack([D.Xs, D.Xs[:1]]))         # d = 4
    try:
        for h in (plain, grad):
            with pytest.raises(api.BossError) as e:
                api.GibbsTrack(h, cand, D.lamS, D.ampS)
            assert e.value.code == api.BOSS_E_INVALID
        with pytest.raises(api.BossError) as e:
            api.GibbsTrack(g, cand, D.lamS, D.ampS)             # unfitted
        assert e.value.code == api.BOSS_E_NOT_FITTED
        D.update(g, 60)
        lib = api.load_library()
        import ctypes as C
        h = C.c_void_p()
        lam4 = np.asfortranarray(np.ones((4, 77)))
        rc = lib.boss_ngp_track_create(g._h, other._h, api._dp(lam4), api._dp(D.ampS), None, C.byref(h))
        assert rc == api.BOSS_E_INVALID and not h.value         # d mismatch
        bad = D.lamS.copy()
        bad[2, 5] = 0.0
        with pytest.raises(api.BossError) as e:
            api.GibbsTrack(g, cand, bad, D.ampS)
        assert e.value.code == api.BOSS_E_INVALID
        bad[2, 5] = -0.3
        with pytest.raises(api.BossError):
            api.GibbsTrack(g, cand, bad, D.ampS)
        tr = api.GibbsTrack(g, cand, D.lamS, D.ampS)            # and the handle still serves a good one
        mu, var = tr.moments()
        ref = g.predict(D.Xs, D.lamS, D.ampS)
        assert np.abs(mu - ref[0]).max() <= 1e-9 and np.abs(np.maximum(var, 0.0) - ref[1]).max() <= 1e-9
        tr.close()
    finally:
        for x in (cand, other, plain, grad, g):
            x.close()


# ------------------------------------------------------------------------------------------ 7: resident latents
def test_latent_form_is_bit_identical(api, O):
    d, N, M = 3, 100, 77
    rng = np.random.default_rng(5)
    Xl = rng.uniform(0, 1, (d, 40))
    yl = 1.5 + 0.3 * np.sin(3 * Xl.sum(0)) + 0.1 * rng.standard_normal(40)
    lg = api.GP(Xl, yl, "matern52")
    lg.update(rng.uniform(0.4, 0.9, d), 1.3, 0.1)
    LAM = ("lognormal", (-1.5, 0.4), "identity", 0.0)
    SAFE = ("lognormal", (-0.7, 0.5), "softplus", 0.1)
    lat = api.NgpLatents([(lg, LAM), 0.45, (lg, LAM)], (lg, SAFE), 0.12)
    X, y, Xs = make(d, N + 2, M, seed=9)
    g = api.GibbsGP(X[:, :N], y[:N])
    cand = api.Candidates(Xs)
    ta = tl = None
    try:
        lamX, ampX, noiX, _, _ = lat.eval(X, jac=False, noise=True)
        g.update(lamX[:, :N], ampX[:N], noiX[:N])
        lamS, ampS, _, _, _ = lat.eval(Xs, jac=False)
        ta = api.GibbsTrack(g, cand, lamS, ampS)
        tl = api.GibbsTrack(g, cand, latents=lat)
        for n in (0, 1, 1):
            if n:
                k = g.N
                g.append(X[:, k:k + 1], y[k:k + 1], lamX[:, k:k + 1], ampX[k:k + 1], noiX[k:k + 1])
            a, b = ta.moments(), tl.moments()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), g.N
        post = O.nonstationary_fit(X, y, lamX, ampX, noiX)
        mu_o, var_o = O.nonstationary_mean_and_var(post, Xs, lamS, ampS, clip=False)
        assert np.abs(b[0] - mu_o).max() <= 1e-9 and np.abs(b[1] - var_o).max() <= 1e-9
        with pytest.raises(api.BossError):                      # a latent object of another x_dim
            api.GibbsTrack(g, cand, latents=api.NgpLatents([0.5, 0.5], 1.0))
    finally:
        for x in (ta, tl):
            if x is not None:
                x.close()
        cand.close()
        g.close()
        lat.close()
        lg.close()


# ------------------------------------------------------------------------------------------ 8: SequentialBatchAM
def test_sequential_batch_equals_the_brute_force_loop(api, O, B):
    """S = 2 samples, P = 2 outputs (EI on output 0 × feasibility of output 1 under a finite y_max): the tracked loop selects what a
    loop of full re-predictions selects, step by step; the top two acquisition values of every step differ by more than 1e-6, so no
    tie decides; the oracle's EI × feasibility at the selected point agrees to 1e-9."""
    from boss_jl_amd.problem import ExperimentData, LinFitness, best_so_far
    d, N, M, S, P, nb = 3, 60, 200, 2, 2, 4
    X, y0, Xs = make(d, N, M, seed=12)
    Y = np.stack([y0, np.cos(2 * X[0]) * 0.5 + 0.1 * np.sin(5 * X[1])])
    coefs, y_max = [1.0, 0.0], [np.inf, 0.45]
    cs = [[1.0, 1.2], [1.1, 0.9]]                               # latent variant of (sample, output)
    mean0 = lambda x: 0.3 * x[0]                                # noqa: E731

    def models():
        out = []
        for s in range(S):
            ls = [latent(d, cs[s][i]) for i in range(P)]
            out.append(B.HipNonstationaryGP([l[0] for l in ls], [l[1] for l in ls], [l[2] for l in ls], [mean0, None]))
        return out

    data = ExperimentData(X.copy(), Y.copy())
    tracked = B.nonstationary_model_posterior_batch(models(), data)
    brute = B.nonstationary_model_posterior_batch(models(), data)
    try:
        sel = B.nonstationary_sequential_batch(tracked, Xs, nb, coefs, y_max, Y)
        assert sel.shape == (d, nb)
        Xa, Ya = X.copy(), Y.copy()
        for k in range(nb):
            best = best_so_far(LinFitness(coefs), Ya, y_max)
            acq, am, mx = B.nonstationary_acq_ei_batch(brute, Xs, coefs, y_max, best)
            top = np.sort(acq)[-2:]
            print(f"step {k}: argmax {am}  max {mx:.6e}  gap {top[1] - top[0]:.2e}", flush=True)
            assert top[1] - top[0] > 1e-6
            x = Xs[:, am]
            assert np.array_equal(sel[:, k], x), (k, am)
            # the oracle on the data so far, closures at every point
            ei_o = 0.0
            for s in range(S):
                mu, var = np.zeros((P, 1)), np.zeros((P, 1))
                for i in range(P):
                    fl, fa, fn = latent(d, cs[s][i])
                    mX = None if i else 0.3 * Xa[0]
                    post = O.nonstationary_fit(Xa, Ya[i], ev(fl, Xa).T, ev(fa, Xa), ev(fn, Xa), mean=mX)
                    mu[i], var[i] = O.nonstationary_mean_and_var(post, x[:, None], ev(fl, x[:, None]).T, ev(fa, x[:, None]),
                                                                 mean_s=None if i else 0.3 * x[:1])
                ei_o += float(O.expected_improvement_lin(coefs, mu, var, best)[0] * O.feas_prob(mu, var, y_max)[0]) / S
            print(f"        oracle {ei_o:.6e}  diff {abs(ei_o - acq[am]):.2e}", flush=True)
            assert abs(ei_o - acq[am]) <= 1e-9
            yhat = np.array([np.mean([brute[s][i].mean_and_var(x)[0] for s in range(S)]) for i in range(P)])
            for row in brute:
                for i, p in enumerate(row):
                    p.append(x, yhat[i])
            Xa = np.concatenate([Xa, x[:, None]], axis=1)
            Ya = np.concatenate([Ya, yhat[:, None]], axis=1)
        for s in range(S):                                      # both sets of slices end on the same data
            for i in range(P):
                assert tracked[s][i].gp.N == brute[s][i].gp.N == N + nb
                assert api._append_path(tracked[s][i].gp) == 1
    finally:
        for row in tracked + brute:
            for p in row:
                p.close()
