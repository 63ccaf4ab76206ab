"""Appends, reserve and tracked candidates of program-kernel posteriors (boss_kgp_set_sequential, api.KernelGP(..., sequential=True),
B.DeviceKernel(f, x_dim, sequential=True)), up to HipSequentialBatchAM over such a model.

Reference: the numpy/scipy restatement of tests/kernel_program_cases.py (Restated: K from the Python closure with the conventions of
include/bosship.h, scipy.linalg.cholesky, solves) on a FRESH fit of all points, at the project's tolerance for this model,
tol = max(1e-9, cond(K)·N·2⁻⁵³·8):  |Δlogpdf| <= tol(1+|logpdf|),  |Δμ| <= tol(1+max|μ|),  |Δσ²| <= tol·max k(x*, x*) — against
_clip_var of the restated σ² for boss_gp_predict, against the UNCLIPPED σ² for tracks.  cond(K) < 1e10 is asserted for every
restatement (the dot-product kernel runs at σ = 0.1, the others at 0.05; the largest observed is printed).
The factor is held to 1e-10·max(1, tol/1e-9): 1e-10 where the tolerance sits on its floor (the bar of the other models' append tests),
growing with cond(K)·N exactly as tol does above it.

Every test fails on the parent commit: the symbol boss_kgp_set_sequential and the keyword `sequential` do not exist there.

Shapes (observations per block row 128, storage in steps of 256 rows, 32 candidates per slab, TRACK_ROWS = 8):
  appends   (d, N0, steps) of the other models' append tests: inside a block, across a block boundary, across a storage boundary
            (with the padding block rows behind), most of the matrix new (re-factorisation), and repeated single observations
            (the rank-one route on the resident inverse factors from the second one on); d = 16 fills the 32 inputs
  tracks    M = 77: three slabs, the last ragged; steps of 9 cross TRACK_ROWS; the 64-instruction program at d = 16 runs one wave
            per workgroup, the exponential kernel at d = 1 four"""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_program_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

AMP = 1.0
M_CAND = 41


def full16(u, v):
    """Matérn-5/2 × inverse multiquadric × squared exponential + squared exponential: 64 instructions at d = 16."""
    r2 = cases._r2(u, v)
    s = np.sqrt(5.0 * r2)
    q = (1 + s + 5.0 / 3.0 * r2) * np.exp(-s)
    return q * (1 / (1 + r2)) * np.exp(-0.125 * r2) + np.exp(-0.5 * r2)


CLOSURES = dict(cases.CLOSURES, full16=full16)


def noise_of(name):
    return 0.1 if name == "dot1" else 0.05


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    B.api.load_library()
    assert B.api.device_count() >= 1
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


_kernels = {}


def kernel_of(B, name, d):
    if (name, d) not in _kernels:
        _kernels[(name, d)] = B.DeviceKernel(CLOSURES[name], d, sequential=True)
    return _kernels[(name, d)]


def clipped(var):
    return np.where((var < 0.0) & (var >= -1e-8), 0.0, var)


class Data:
    """Points, targets, candidates, hyper-parameters and (optionally) a prior mean and one discrete dimension of a case."""

    def __init__(self, name, d, Ntot, M, mean, disc, seed=21, c=1.0):
        self.name, self.d, self.f = name, d, CLOSURES[name]
        sc = np.ones(d)
        self.discrete = None
        if disc:
            self.discrete = np.zeros(d, bool)
            self.discrete[1] = True
            sc[1] = 5.0
        self.X, self.y, self.Xs = cases.data(d, Ntot, M, seed=seed + d, scale=sc)
        self.lam = np.linspace(0.4, 0.6, d) * sc * c          # c != 1: "other hyper-parameters" at the same points
        self.amp, self.sig = AMP * c, noise_of(name) * c
        self.mX = 0.5 + 0.2 * self.X.sum(0) if mean else None
        self.mS = 0.5 + 0.2 * self.Xs.sum(0) if mean else None

    def m(self, a, b):
        return None if self.mX is None else self.mX[a:b]

    def handle(self, B, N, sequential=True):
        return B.api.KernelGP(self.X[:, :N], self.y[:N], kernel_of(B, self.name, self.d).program, self.discrete, sequential=sequential)

    def builtin(self, api, N):
        return api.GP(self.X[:, :N], self.y[:N], "matern52", self.discrete)

    def update(self, g, N):
        return g.update(self.lam, self.amp, self.sig, self.m(0, N))

    def append(self, g, a, b):
        return g.append(self.X[:, a:b], self.y[a:b], self.m(a, b))

    def restated(self, N):
        ref = cases.Restated(self.f, self.X[:, :N], self.y[:N], self.lam, self.amp, self.sig, self.Xs, self.discrete, self.m(0, N), self.mS)
        assert ref.cond < 1e10, ref.cond
        return ref

    def check(self, g, lp, N, what):
        """logpdf and the clipped moments of boss_gp_predict against a fresh restatement of the first N points."""
        ref = self.restated(N)
        mu, var = g.predict(self.Xs, self.mS)
        report(what, ref, lp, mu, var, clipped(ref.var))
        assert g.N == N
        return ref


def report(what, ref, lp, mu, var, var_ref):
    tol = ref.tol
    e_mu, e_var = np.abs(mu - ref.mu).max(), np.abs(var - var_ref).max()
    line = f"[kseq] {what}: cond {ref.cond:.3e} tol {tol:.3e}"
    if lp is not None:
        line += f" |dlogpdf| {abs(lp - ref.logpdf):.3e} (bound {tol * (1 + abs(ref.logpdf)):.3e})"
    print(line + f" |dmu| {e_mu:.3e} (bound {tol * (1 + np.abs(ref.mu).max()):.3e}) |dvar| {e_var:.3e} (bound {tol * ref.kss.max():.3e})",
          flush=True)
    if lp is not None:
        assert abs(lp - ref.logpdf) <= tol * (1 + abs(ref.logpdf)), what
    assert e_mu <= tol * (1 + np.abs(ref.mu).max()), what
    assert e_var <= tol * ref.kss.max(), what


# ------------------------------------------------------------------------------------------ 1: append parity
APPEND_CASES = [(3, 5, [1, 1, 3]), (3, 127, [2]), (3, 128, [1]), (3, 255, [1, 130]), (3, 250, [7, 300]), (3, 256, [600]), (16, 130, [1, 1, 1])]
APPEND_PARAMS = [(d, N0, st, mean, disc) for d, N0, st in APPEND_CASES for mean in (False, True) for disc in ((False, True) if d == 3 else (False,))]
# the routes the issue names: 3 (rank-one on resident inverses) from the second single append on, 2 (re-factorisation) where most is new
ROUTES = {(3, 5): [1, 3, 3], (16, 130): [1, 3, 3], (3, 127): [2], (3, 256): [2], (3, 128): [1]}


@pytest.mark.parametrize("name", ["expo", "dot1", "persq"])
@pytest.mark.parametrize("d,N0,steps,mean,disc", APPEND_PARAMS)
def test_append_parity(B, api, name, d, N0, steps, mean, disc):
    """After every step logpdf, μ, σ² at 41 candidates against a fresh restatement of all points, and the route of the append equal to
    the one a built-in Matérn-5/2 handle takes through the same create / update / append sequence; at the end the factor, then a full
    update at other hyper-parameters on the grown handle against a fresh restatement."""
    Nt = N0 + sum(steps)
    D = Data(name, d, Nt, M_CAND, mean, disc)
    g, gb = D.handle(B, N0), D.builtin(api, N0)
    try:
        assert api._append_path(g) == 0
        D.update(g, N0)
        D.update(gb, N0)
        N, routes = N0, []
        for n in steps:
            lp = D.append(g, N, N + n)
            D.append(gb, N, N + n)
            N += n
            ref = D.check(g, lp, N, f"{name} d={d} N0={N0} +{n} mean={mean} disc={disc}")
            routes.append(api._append_path(g))
            assert routes[-1] == api._append_path(gb) and routes[-1] in (1, 2, 3), (N, n, routes, api._append_path(gb))
        if (d, N0) in ROUTES:
            assert routes == ROUTES[(d, N0)], routes
        if name == "dot1":
            assert np.ptp(ref.kss) > 0.1 * ref.kss.max()         # the prior variance differs from point to point
        L, z = g.factor()
        eL, bL = np.abs(L - ref.L).max(), 1e-10 * max(1.0, ref.tol / 1e-9)
        print(f"[kseq] factor {eL:.2e} (bound {bL:.2e}) z {np.abs(z - ref.z).max():.2e}", flush=True)
        assert eL <= bL
        D2 = Data(name, d, Nt, M_CAND, mean, disc, c=1.15)
        lp = D2.update(g, Nt)
        D2.check(g, lp, Nt, "update on the grown handle")
    finally:
        g.close()
        gb.close()


# ------------------------------------------------------------------------------------------ 2: the old blocks are untouched
def test_block_row_leaves_old_blocks_bit_identical(B, api):
    D = Data("dot1", 3, 301, M_CAND, True, False)
    g = D.handle(B, 300)
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


@pytest.mark.parametrize("name", ["expo", "dot1"])
def test_refactorising_append_equals_a_fresh_handle_bit_for_bit(B, api, name):
    D = Data(name, 3, 129, M_CAND, True, False)
    g, fresh = D.handle(B, 127), D.handle(B, 129)
    try:
        D.update(g, 127)
        lp = D.append(g, 127, 129)
        assert api._append_path(g) == 2
        lpf = D.update(fresh, 129)
        (mu, var), (muf, varf) = g.predict(D.Xs, D.mS), fresh.predict(D.Xs, D.mS)
        assert lp == lpf and np.array_equal(mu, muf) and np.array_equal(var, varf)
    finally:
        g.close()
        fresh.close()


# ------------------------------------------------------------------------------------------ 3: reserve
def test_reserve_then_single_appends(B, api):
    """N0 = 250 in 256 rows of storage; reserve(262) grows it once.  Without it the seventh observation would: a growth re-lays the
    arrays out and drops the inverse factors, so that append would run as block rows (route 1).  Routes [1, 3 × 11] therefore show that
    no append grew the storage."""
    N0, n = 250, 12
    D = Data("dot1", 3, N0 + n, M_CAND, True, False)
    g = D.handle(B, N0)
    try:
        D.update(g, N0)
        g.reserve(N0 + n)
        with pytest.raises(api.BossError) as e:                  # reserve leaves the handle unfitted
            D.append(g, N0, N0 + 1)
        assert e.value.code == api.BOSS_E_NOT_FITTED and g.N == N0
        lp = D.update(g, N0)
        D.check(g, lp, N0, "update after reserve")
        routes = []
        for j in range(n):
            lp = D.append(g, N0 + j, N0 + j + 1)
            routes.append(api._append_path(g))
            D.check(g, lp, N0 + j + 1, f"reserved +{j + 1}")
        assert routes == [1] + [3] * (n - 1), routes
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 4: tracks
TRACK_CASES = [("dot1", 3, 100, [1, 1, 1], True, False), ("expo", 3, 250, [3, 9, 1], False, True), ("persq", 16, 120, [8, 9], False, False),
               ("full16", 16, 120, [3, 9], True, False), ("expo", 1, 100, [2, 9], False, False)]


def test_the_track_programs_cover_both_ends_of_the_workgroup_sizing(B):
    """kprog_block: as many of 4 waves as fit 64 KiB at 8·64·(2d + n_instr) bytes per wave (tests/test_gpu_kernel_program_batch.py)."""
    waves = lambda p: max(1, min(4, 65536 // (8 * 64 * (2 * p.d + p.code.shape[0]))))   # noqa: E731
    short, full = kernel_of(B, "expo", 1).program, kernel_of(B, "full16", 16).program
    assert short.code.shape[0] == 5 and waves(short) == 4
    assert full.code.shape[0] == B.api.FIT_MAX_INSTR == 64 and waves(full) == 1


@pytest.mark.parametrize("name,d,N0,steps,mean,disc", TRACK_CASES)
def test_tracks(B, api, name, d, N0, steps, mean, disc):
    M = 77                                                      # three slabs, the last ragged
    Nt = N0 + sum(steps)
    D = Data(name, d, Nt, M, mean, disc)
    g = D.handle(B, N0)
    cand = api.Candidates(D.Xs)
    tr = None
    try:
        D.update(g, N0)
        tr = api.Track(g, cand, D.mS)
        coefs, y_max, best = [1.0], [0.4], 0.2
        N = N0
        for n in [0] + steps:
            if n:
                D.append(g, N, N + n)
                N += n
            mu, var = tr.moments()
            ref = D.restated(N)
            report(f"track {name} d={d} N={N}", ref, None, mu, var, ref.var)   # the UNCLIPPED restated σ²
            acq, am, mx = api.acq_ei_tracks([[tr]], coefs, y_max, best)
            acq_m, am_m, mx_m = api.acq_ei_moments(mu[None, None, :], var[None, None, :], coefs, y_max, best)
            assert np.abs(acq - acq_m).max() <= 1e-12 and am == am_m
            tr.sync()
            again = tr.moments()
            tr.sync()
            again2 = tr.moments()
            assert np.array_equal(again[0], mu) and np.array_equal(again[1], var)
            assert np.array_equal(again2[0], mu) and np.array_equal(again2[1], var)
        D2 = Data(name, d, Nt, M, mean, disc, c=1.15)
        D2.update(g, Nt)                                        # other hyper-parameters: the track is stale
        with pytest.raises(api.BossError) as e:
            tr.sync()
        assert e.value.code == api.BOSS_E_INVALID
        with pytest.raises(api.BossError) as e:
            tr.moments()
        assert e.value.code == api.BOSS_E_INVALID
    finally:
        if tr is not None:
            tr.close()
        cand.close()
        g.close()


# ------------------------------------------------------------------------------------------ 5: a member of a fitted set
def test_set_member_leaves_its_set(B, api):
    S, N = 3, 140
    Ds = [Data("dot1", 3, N + 1, M_CAND, True, False, c=c) for c in (1.0, 1.1, 1.2)]
    D0 = Ds[0]
    lam = np.stack([D.lam for D in Ds], axis=1)
    gps, _, st = api.kgp_fit_batch(D0.X[:, :N], D0.y[:N], kernel_of(B, "dot1", 3).program, lam, [D.amp for D in Ds], [D.sig for D in Ds],
                                   D0.mX[:N], None, sequential=True)
    try:
        assert np.all(st == api.BOSS_OK) and all(g.sequential for g in gps)
        before = [g.predict(D.Xs, D.mS) for g, D in zip(gps, Ds)]
        lp = Ds[1].append(gps[1], N, N + 1)
        assert api._append_path(gps[1]) == 1
        for s in (0, 2):
            after = gps[s].predict(Ds[s].Xs, Ds[s].mS)
            assert np.array_equal(after[0], before[s][0]) and np.array_equal(after[1], before[s][1]), s
            assert gps[s].N == N
        Ds[1].check(gps[1], lp, N + 1, "set member")
    finally:
        for g in gps:
            g.close()


# ------------------------------------------------------------------------------------------ 6: the switch
def test_the_switch(B, api):
    D = Data("expo", 3, 131, M_CAND, False, False)
    lib = api.load_library()
    flagged, plain, builtin = D.handle(B, 130), D.handle(B, 130, sequential=False), D.builtin(api, 130)
    cand = api.Candidates(D.Xs)
    try:
        for h in (flagged, plain, builtin):
            D.update(h, 130)
        ref_plain, ref_flagged = plain.predict(D.Xs), flagged.predict(D.Xs)
        assert np.array_equal(ref_plain[0], ref_flagged[0]) and np.array_equal(ref_plain[1], ref_flagged[1])   # the flag changes no result

        def refused(h):
            for what, call in (("append", lambda: D.append(h, 130, 131)), ("reserve", lambda: h.reserve(200)), ("Track", lambda: api.Track(h, cand))):
                with pytest.raises(api.BossError) as e:
                    call()
                assert e.value.code == api.BOSS_E_INVALID and "program-kernel posteriors" in str(e.value), (what, str(e.value))
            assert h.N == 130
        refused(plain)
        again = plain.predict(D.Xs)
        assert np.array_equal(again[0], ref_plain[0]) and np.array_equal(again[1], ref_plain[1])
        # a flagged handle takes the three calls (a track first: reserve leaves a handle unfitted)
        tr = api.Track(flagged, cand)
        mu, var = tr.moments()
        tr.close()
        assert np.abs(mu - ref_flagged[0]).max() <= 1e-9
        # ... and is still refused where every program handle is
        assert api.init() >= 1
        for what, call in (("update_acq", lambda: flagged.update_acq(D.lam, D.amp, D.sig, cand)),
                           ("predict_cov", lambda: flagged.predict_cov(D.Xs[:, :3])),
                           ("multi_update", lambda: api.multi_update([flagged], D.lam, D.amp, D.sig))):
            with pytest.raises(api.BossError) as e:
                call()
            assert e.value.code == api.BOSS_E_INVALID and "program-kernel posteriors" in str(e.value), (what, str(e.value))
        # off again: the refusals are back and nothing it computes has changed; independent of the gradient flag
        assert lib.boss_kgp_set_sequential(flagged._h, 0) == api.BOSS_OK
        refused(flagged)
        again = flagged.predict(D.Xs)
        assert np.array_equal(again[0], ref_flagged[0]) and np.array_equal(again[1], ref_flagged[1])
        assert lib.boss_kgp_set_grad(flagged._h, 1) == api.BOSS_OK
        refused(flagged)
        assert lib.boss_kgp_set_sequential(flagged._h, 1) == api.BOSS_OK and lib.boss_kgp_set_grad(flagged._h, 0) == api.BOSS_OK
        with pytest.raises(api.BossError, match="boss_kgp_set_grad"):
            flagged.predict_grad(D.Xs[:, :3])
        lp = D.append(flagged, 130, 131)                         # after the update, as before it
        D.check(flagged, lp, 131, "switched on after the update")
        # the switch itself: built-in handles and NULL
        for on in (0, 1):
            assert lib.boss_kgp_set_sequential(builtin._h, on) == api.BOSS_E_INVALID
            assert b"was not created by boss_kgp_create" in lib.boss_last_error()
            assert lib.boss_kgp_set_sequential(None, on) == api.BOSS_E_INVALID
        lpb = D.append(builtin, 130, 131)                        # the built-in handle appends as it always did
        assert np.isfinite(lpb) and api._append_path(builtin) == 1
    finally:
        cand.close()
        for h in (flagged, plain, builtin):
            h.close()


# ------------------------------------------------------------------------------------------ 7: HipSequentialBatchAM
SEQ = dict(d=2, N=60, M=200, P=2, nb=4, seed=17, coefs=[1.0, 0.25], y_max=[np.inf, 0.6], beta=2.0)
GAP = 1e-6


def seq_inputs():
    rng = np.random.default_rng(SEQ["seed"])
    d, N, M = SEQ["d"], SEQ["N"], SEQ["M"]
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1]])
    Xs = np.asfortranarray(rng.uniform(0, 1, (d, M)))
    lam = [np.array([[0.3, 0.5], [0.4, 0.6]]), np.array([[0.36, 0.55], [0.44, 0.7]])]
    amp, sig = [[1.0, 0.8], [1.1, 0.9]], [[0.1, 0.1], [0.12, 0.1]]
    return X, Y, Xs, lam, amp, sig


def seq_values(O, kind, mu, var, Yo):
    """The acquisition of one pick from the S×P×M moments: the EI × feasibility of expected_improvement.jl:77-90 averaged over the
    samples, or the upper confidence bound cᵀμ + β sqrt((c²)ᵀσ²) likewise."""
    c = np.asarray(SEQ["coefs"], float)
    if kind == "ucb":
        return np.mean([c @ m + SEQ["beta"] * np.sqrt((c * c) @ v) for m, v in zip(mu, var)], axis=0)
    best = O.best_so_far(c, Yo, SEQ["y_max"])
    return np.mean([O.expected_improvement_lin(c, m, v, best) * O.feas_prob(m, v, SEQ["y_max"]) for m, v in zip(mu, var)], axis=0)


def restated_loop(O, name, kind, S):
    """The reference's loop (batch.jl:26-38) on restatements alone: (picks, smallest relative gap between the best and the second-best
    acquisition value over the picks).  No device."""
    X, Y, Xs, lam, amp, sig = seq_inputs()
    f, P = CLOSURES[name], SEQ["P"]
    Xo, Yo, picks, gap = X.copy(), Y.copy(), [], np.inf
    for _ in range(SEQ["nb"]):
        refs = [[cases.Restated(f, Xo, Yo[i], lam[s][:, i], amp[s][i], sig[s][i], Xs, want_cond=False) for i in range(P)] for s in range(S)]
        mu = np.array([[r.mu for r in row] for row in refs])
        var = np.array([[clipped(r.var) for r in row] for row in refs])
        acq = seq_values(O, kind, mu, var, Yo)
        order = np.argsort(acq)
        gap = min(gap, (acq[order[-1]] - acq[order[-2]]) / abs(acq[order[-1]]))
        j = int(order[-1])
        picks.append(j)
        Xo = np.hstack([Xo, Xs[:, j:j + 1]])
        Yo = np.hstack([Yo, mu[:, :, j].mean(0)[:, None]])
    return picks, gap


def seq_problem(B, name, kind, S):
    X, Y, Xs, lam, amp, sig = seq_inputs()
    P = SEQ["P"]
    prms = [B.HipGPParams(lam[s], amp[s], sig[s]) for s in range(S)]
    model = B.HipGaussianProcess([None] * P, [None] * P, [None] * P, kernel=kernel_of(B, name, SEQ["d"]))
    fit = B.LinFitness(SEQ["coefs"])
    acq = B.UpperConfidenceBound(fit, SEQ["beta"]) if kind == "ucb" else B.ExpectedImprovement(fit)
    prob = B.BossProblem(None, B.Domain((np.zeros(SEQ["d"]), np.ones(SEQ["d"]))), acq, model, B.ExperimentData(X, Y), SEQ["y_max"],
                         prms[0] if S == 1 else prms)
    return prob, Xs


def brute_force(B, prob, Xs):
    """HipBatchAM on a fresh model_posterior of the augmented data for every pick (what the parent commit can do with such a model);
    the gap between the best and the second-best value is asserted at every pick, so a tie cannot hide a wrong pick."""
    from boss_jl_amd.maximizer import posteriors_of
    pr = copy.copy(prob)
    pr.data = type(prob.data)(prob.data.X.copy(), prob.data.Y.copy())
    picks = []
    for k in range(SEQ["nb"]):
        _, acq = B.HipBatchAM(points=Xs).maximize_acquisition(pr, return_all=True)
        order = np.argsort(acq)
        gap = (acq[order[-1]] - acq[order[-2]]) / abs(acq[order[-1]])
        print(f"[kseq] brute-force pick {k}: column {order[-1]} value {acq[order[-1]]:.6e} relative gap {gap:.3e}", flush=True)
        assert gap >= GAP, (k, gap)
        j = int(order[-1])
        posts = posteriors_of(pr)
        try:
            y = sum(p.mean(Xs[:, j]) for p in posts) / len(posts)
        finally:
            for p in posts:
                p.close()
        pr.augment_dataset(Xs[:, j], y)
        picks.append(j)
    return picks


@pytest.mark.parametrize("name", ["expo", "dot1"])
@pytest.mark.parametrize("kind,S", [("ei", 1), ("ucb", 1), ("ei", 2)])
def test_sequential_batch_am_selects_the_brute_force_columns(B, O, name, kind, S):
    """kind = ei: the tracked route (fixed candidates, LinFitness, shard = candidates), with one parameter set and with a list of two
    (BI samples); kind = ucb: the untracked loop through a DeviceAcquisition.  The model carries ONE kernel for its P = 2 outputs, so
    the two closures of the issue are two runs."""
    prob, Xs = seq_problem(B, name, kind, S)
    want_cpu, gap_cpu = restated_loop(O, name, kind, S)
    print(f"[kseq] {name} {kind} S={S}: restated picks {want_cpu}, smallest relative gap {gap_cpu:.3e}", flush=True)
    assert gap_cpu >= GAP                                        # the condition on the inputs, on the restatement alone
    want = brute_force(B, prob, Xs)
    assert want == want_cpu
    xs, val = B.HipSequentialBatchAM(B.HipBatchAM(points=Xs), SEQ["nb"]).maximize_acquisition(prob)
    assert val is None and xs.shape == (SEQ["d"], SEQ["nb"])
    assert [int(np.flatnonzero(np.all(Xs == xs[:, [k]], axis=0))[0]) for k in range(SEQ["nb"])] == want
    assert prob.data.X.shape[1] == SEQ["N"]                      # the caller's problem is untouched
    if kind == "ei" and S == 1:                                  # the untracked loop of the same acquisition: shard = outputs
        xs2, _ = B.HipSequentialBatchAM(B.HipBatchAM(points=Xs, shard="outputs"), SEQ["nb"]).maximize_acquisition(prob)
        assert np.array_equal(xs2, xs)


def test_python_surface_of_a_flagged_model(B, api):
    """slice.append, post.append and model_posterior(..., reserve=…) with a closure prior mean; cov keeps raising; an unflagged model
    keeps refusing with the message that names the switch."""
    X, Y, Xs, lam, amp, sig = seq_inputs()
    P = SEQ["P"]
    mean = lambda x: [0.1 + 0.2 * x[0], -0.2]                    # noqa: E731
    model = B.HipGaussianProcess([None] * P, [None] * P, [None] * P, mean=mean, kernel=kernel_of(B, "dot1", 2))
    prm = B.HipGPParams(lam[0], amp[0], sig[0])
    N = SEQ["N"]
    post = model.model_posterior(prm, B.ExperimentData(X[:, :N - 2], Y[:, :N - 2]), reserve=2)
    try:
        post.append(X[:, N - 2], Y[:, N - 2])
        for i, s in enumerate(post.slices):
            s.append(X[:, N - 1], Y[i, N - 1])
        mu, var = post.mean_and_var(Xs[:, :M_CAND])
        for i in range(P):
            mX, mS = np.array([mean(X[:, j])[i] for j in range(N)]), np.array([mean(Xs[:, j])[i] for j in range(M_CAND)])
            ref = cases.Restated(cases.dot1, X, Y[i], lam[0][:, i], amp[0][i], sig[0][i], Xs[:, :M_CAND], None, mX, mS)
            assert ref.cond < 1e10
            report(f"python surface output {i}", ref, post.slices[i].gp.logpdf, mu[i], var[i], clipped(ref.var))
        with pytest.raises(NotImplementedError, match="DeviceKernel"):
            post.cov(Xs[:, :3])
    finally:
        post.close()
    plain = B.HipGaussianProcess([None] * P, [None] * P, [None] * P, kernel=B.DeviceKernel(cases.dot1, 2))
    with pytest.raises(NotImplementedError, match="sequential=True"):
        plain.model_posterior(prm, B.ExperimentData(X, Y), reserve=2)
