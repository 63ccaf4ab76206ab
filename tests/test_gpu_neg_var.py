"""The negative-variance convention on every prediction path (pytest -m gpu): _clip_var (gaussian_process.jl:186-194) as
include/bosship.h promises it — a variance in [-1e-8, 0) comes back as exactly 0; below that the prediction calls fail with
BOSS_E_NEG_VAR, *bad_index = the FIRST offending candidate, "mu/var are still written (var unclipped at the offending entries)", and
the acquisition calls make the candidate -Inf with a zero gradient (SafeFunction, src/acquisition.jl:21-25).

Two constructions (tests/neg_var_cases.py; their inputs are measured on the CPU by tests/test_neg_var_host.py):

A, exact, on program-kernel handles: a traced kernel whose prior variance is chosen per candidate puts variances at -0.99e-8, -5e-9
   (exactly 0.0 expected), -1.01e-8, -2e-8 (offending, returned unclipped) and +5e-9 with no substitution error, next to healthy
   candidates and to one that offends by a wide margin, held to the restatement with the project bars
   tol = max(1e-9, cond·N·2⁻⁵³·8): |Δμ| <= tol(1 + max|μ|), |Δσ²| <= tol·max k(x*, x*).  Shapes:
     n20     N = 20,   M = 12      offenders 5, 9           not the built-in one-launch path
     n130    N = 130,  M = 70      offenders 37, 69         predict_kernel<G32, true>, ragged tile
     n130b   N = 130,  M = 16389   offenders 9000, 16388    predict_kernel<G64, true> slabs, last ragged slab; 65 blocks of clip_var_kernel
     n130a3  the n130 shape at α = 3
     n1030   N = 1030, M = 40      offenders 33, 35, 38     few-candidates route: the step path, then the inverse-GEMM finish;
                                                            M = 3 (healthy, in-band, offender): winv_finish_kernel
B, rounding-driven, for the paths a program handle cannot reach (built-in kernels, d = 1, α = 1e5, σ = 1e-4, candidates = 37
   midpoints, then the training points): which training-point candidates offend depends on the summation order, so every call is held
   to the contract on what it returns — C1: rc == BOSS_E_NEG_VAR iff a returned variance is below -1e-8, bad_index the smallest such
   index; C2: no returned entry in [-1e-8, 0); C3: |Δμ| <= B(1 + max|μ|), |Δσ²| <= B·α², B = 8·cond·N·2⁻⁵³ (the bars of
   tests/test_gpu_regimes.py, no floor) against the float64 restatement; C4: an offender and a non-offending training-point
   candidate exist and no midpoint offends (no test passes vacuously).
   An equal offender set between two calls is required only where the header or DESIGN.md states bit-for-bit agreement (quoted there).

Every call prints its route, the number of offenders, bad_index and the largest deviation in units of its bar."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import kernel_program_cases as K  # noqa: E402
import neg_var_cases as NV  # noqa: E402

pytestmark = pytest.mark.gpu

PRUNED = 1                                                   # boss_debug_acq_path's report of a pruned call
BEST_A = -0.25                                               # below μ = 0 of the far candidates: a clipped one has EI = 0.25, not 0
EPS = 2.0 ** -52


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


_kernels, _handles = {}, {}


def kernel_of(B, f, d=3):
    if (f, d) not in _kernels:
        _kernels[(f, d)] = B.DeviceKernel(f, d)
    return _kernels[(f, d)]


def fitted_a(B, c):
    """one fitted program-kernel handle per (N, α), shared by the tests (none changes its factorisation's numbers)"""
    key = ("A", c.N, c.amp)
    if key not in _handles:
        g = B.api.KernelGP(c.X, c.y, kernel_of(B, NV.flagged).program)
        g.update(c.lam, c.amp, c.sig)
        _handles[key] = g
    return _handles[key]


def fitted_b(api, c):
    key = ("B", c.N, c.kernel, c.seed)
    if key not in _handles:
        g = api.GP(c.X, c.y, c.kernel)
        g.update(c.lam, c.amp, c.sig)
        _handles[key] = g
    return _handles[key]


def ints(a):
    return [int(v) for v in a]


def worst(got, want, bar):
    """Largest |got − want| in units of its bar; entries with bar 0 must match exactly (0.0 == -0.0)."""
    got, want, bar = np.asarray(got, float), np.asarray(want, float), np.asarray(bar, float)
    exact = bar == 0.0
    assert np.array_equal(got[exact], want[exact]), (np.flatnonzero(exact)[got[exact] != want[exact]][:8], got[exact][got[exact] != want[exact]][:8])
    return float((np.abs(got - want)[~exact] / bar[~exact]).max()) if (~exact).any() else 0.0


def check_a(tag, route, api, rc, bad, mu, var, want_mu, want_var, bar_mu, bar_var, off):
    noff = NV.offenders(var)
    r_mu, r_var = worst(mu, want_mu, bar_mu), worst(var, want_var, bar_var)
    print(f"[negvar] A {tag}: route {route} rc {rc} bad_index {bad} offenders {ints(noff[:6])} |dmu| {r_mu:.3f} |dvar| {r_var:.3f} of their bars")
    assert r_mu <= 1.0 and r_var <= 1.0
    assert list(noff) == list(off)
    assert (rc, bad) == ((api.BOSS_E_NEG_VAR, off[0]) if len(off) else (api.BOSS_OK, -1))
    NV.contract(api, rc, bad, var)


ROUTE_A = {"n20": "tiled G32 (N <= 128, not the one-launch path)", "n130": "G32", "n130b": "G64 slabs", "n130a3": "G32, alpha 3"}


# ------------------------------------------------------------------------------------------ A1, A2: boss_gp_predict
@pytest.mark.parametrize("name", ["n20", "n130", "n130b", "n130a3"])
def test_a_predict_clean_and_poisoned(B, api, name):
    c = NV.case_a(name)
    assert c.ref.cond < 1e6
    g = fitted_a(B, c)
    clean = NV.predict_raw(api, g, c.Xs_clean)
    check_a(f"{name} clean", ROUTE_A[name], api, *clean, c.want_mu_clean, c.want_var_clean, c.bar_mu_clean, c.bar_var_clean, [])
    first = NV.predict_raw(api, g, c.Xs)
    check_a(f"{name} poisoned", ROUTE_A[name], api, *first, c.want_mu, c.want_var, c.bar_mu, c.bar_var, c.off)
    again = NV.predict_raw(api, g, c.Xs)                     # "The kernels hold no atomics: repeated calls agree bit for bit." (bosship.h, boss_kgp_create)
    assert again[:2] == first[:2] and np.array_equal(again[2], first[2]) and np.array_equal(again[3], first[3])
    after = NV.predict_raw(api, g, c.Xs_clean)               # a clean call after a failed one succeeds, with the same bits as before it
    assert after[:2] == (api.BOSS_OK, -1) and np.array_equal(after[2], clean[2]) and np.array_equal(after[3], clean[3])
    # the columns rotated by one, and the last offender moved to entry 0: bad_index follows the first offender
    if c.M <= 256:
        for perm in (list(range(1, c.M)) + [0], [c.off[-1]] + [j for j in range(c.M) if j != c.off[-1]]):
            Xp, wm, wv, bm, bv, off = c.columns(perm)
            check_a(f"{name} permuted, first offender {off[0]}", ROUTE_A[name], api, *NV.predict_raw(api, g, Xp), wm, wv, bm, bv, off)


def test_a_few_candidates_route_and_its_resident_inverse_finishes(B, api):
    """N = 1030 (Np = 1280), as tests/test_gpu_kernel_program.py reaches the finishes: the step path first, from the
    BOSS_WINV_AFTER-th call on one factorisation the inverse GEMMs (inv_fwd_finish_kernel) for M = 40 and the one pass over L⁻ᵀ
    (winv_finish_kernel) for M = 3; the route is read from the handle's counters."""
    for knob in ("BOSS_INVGEMM_MAX_TILES", "BOSS_FEW_MAX_TILES", "BOSS_NO_FEW"):
        assert os.environ.get(knob) is None, knob + " is set: this test would not reach the resident-inverse finishes"
    winv_after = int(os.environ.get("BOSS_WINV_AFTER", "2"))
    assert winv_after >= 1, "BOSS_WINV_AFTER=0 switches the resident inverses off"
    c = NV.case_a("n1030")
    assert c.ref.cond < 1e6
    g = fitted_a(B, c)
    sets = {40: (c.Xs, c.want_mu, c.want_var, c.bar_mu, c.bar_var, c.off), 3: c.columns(NV.N1030_M3)}
    assert sets[3][5] == [2]
    for M, (Xs, wm, wv, bm, bv, off) in sets.items():
        g.update(c.lam, c.amp, c.sig)                        # a new factorisation (the same numbers): the call count starts over
        assert api._acq_counters(g)[:2] == (0, 0)
        seen = []
        for rep in range(winv_after + 2):
            res = NV.predict_raw(api, g, Xs)
            have_winv, few_calls = api._acq_counters(g)[:2]
            assert have_winv == (1 if rep + 1 >= winv_after else 0) and few_calls == min(rep + 1, winv_after), (rep, have_winv, few_calls)
            route = "step path" if not have_winv else ("inverse-GEMM finish" if M > 4 else "winv_finish_kernel")
            check_a(f"n1030 M={M} call {rep}", route, api, *res, wm, wv, bm, bv, off)
            seen.append(res)
        assert np.array_equal(seen[-1][3], seen[-2][3]) and np.array_equal(seen[-1][2], seen[-2][2])      # one path twice: the same bits
    clean = NV.predict_raw(api, g, c.Xs_clean)
    check_a("n1030 clean", "inverse-GEMM finish", api, *clean, c.want_mu_clean, c.want_var_clean, c.bar_mu_clean, c.bar_var_clean, [])


# ------------------------------------------------------------------------------------------ A3 .. A5: boss_acq_ei
def ei_expected(O, want_mu, want_var, bar_mu, bar_var, off, best):
    """(EI per candidate with -Inf at the offenders, bound per candidate): the bound of test_acq_ei_over_outputs_and_samples
    (tests/test_gpu_kernel_program.py) taken per candidate — |ΔE| <= Δμ + 0.4·Δσ²/(2σ) (∂EI/∂μ = Φ <= 1, ∂EI/∂σ = φ <= 0.4,
    Δσ <= Δσ²/(2σ)) with the candidate's own bars; a clipped candidate (σ = 0 on both sides) has |ΔE| <= Δμ.  8·2⁻⁵²(1 + |E|) is
    added for the epilogue's own roundings (Φ, φ, two products and a sum), which the bars of an exact candidate do not cover."""
    v = np.where(np.isin(np.arange(want_mu.size), off), 1.0, want_var)
    want = O.expected_improvement_lin([1.0], want_mu[None, :], v[None, :], best)
    s = np.sqrt(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = bar_mu + np.where(s > 0.0, 0.4 * bar_var / (2 * s), 0.0) + 8 * EPS * (1 + np.abs(want))
    want = want.copy()
    want[off] = -np.inf
    return want, bound


@pytest.mark.parametrize("name", ["n20", "n130", "n130b", "n130a3", "n1030"])
def test_a_acq_ei(B, api, O, name):
    c = NV.case_a(name)
    g = fitted_a(B, c)
    want, bound = ei_expected(O, c.want_mu, c.want_var, c.bar_mu, c.bar_var, c.off, BEST_A)
    cand = api.Candidates(c.Xs)
    try:
        acq, am, mx = api.acq_ei([[g]], cand, [1.0], None, BEST_A)
        _, am2, mx2 = api.acq_ei([[g]], cand, [1.0], None, BEST_A, want_acq=False)
    finally:
        cand.close()
    inf = np.flatnonzero(np.isneginf(acq))
    fin = np.setdiff1d(np.arange(c.M), c.off)
    clip = np.flatnonzero(c.far & (c.want_var == 0.0))
    print(f"[negvar] A acq_ei {name}: counters {api._acq_counters(g)[:2]} -Inf at {ints(inf)} argmax {am} / {int(np.argmax(want))} max {mx!r} "
          f"max|dacq|/bound {(np.abs(acq[fin] - want[fin]) / bound[fin]).max():.3e} EI at the clipped candidates {[float(v) for v in acq[clip]]}")
    assert list(inf) == c.off and np.isfinite(acq[fin]).all()
    assert np.all(np.abs(acq[fin] - want[fin]) <= bound[fin])
    assert np.all(np.abs(acq[clip] - (0.0 - BEST_A)) <= 8 * EPS * (1 - BEST_A))      # the EI of σ = 0 at μ = 0: μ − best
    assert am == int(np.argmax(want)) and am not in c.off and mx == acq[am]
    assert (am2, mx2) == (am, mx)


def test_a_acq_ei_over_outputs_and_samples(B, api, O):
    """P = 2 (y_max = [inf, 0.5]), S = 2, only member (s = 1, p = 1) on `flagged`, the others on the exponential kernel: the sample mean
    is -Inf where any sample is, elsewhere within the bound of test_acq_ei_over_outputs_and_samples taken per candidate and member:
    E = EI of output 0, F = Φ((y_max − μ₁)/σ₁), |ΔE| <= Δμ₀ + 0.4·Δσ²₀/(2σ₀), |ΔF| <= 0.4·Δμ₁/σ₁ + 0.242·Δσ²₁/(2σ₁²),
    |Δacq_s| <= |ΔE| + E·|ΔF|, the mean over samples no larger.  A clipped far candidate of the flagged member has μ₁ = 0 and σ₁ = 0
    exactly on both sides: F = 1, ΔF = 0."""
    c = NV.case_a("n130")
    Y = np.stack([c.y, 0.4 + 0.3 * np.cos(3.0 * c.X[:2].sum(0))])
    coefs, y_max = [1.0, 0.0], [np.inf, 0.5]
    gps, acqs, bounds = [], [], []
    poisoned = np.zeros(c.M, bool)
    try:
        for s in range(2):
            row, mus, vars_, bms, bvs = [], [], [], [], []
            for p in range(2):
                f = NV.flagged if (s, p) == (1, 1) else K.expo
                lam = c.lam if f is NV.flagged else c.lam * (1.0 + 0.15 * s)
                sig = c.sig if f is NV.flagged else c.sig * (1.0 + 0.2 * s)
                g = api.KernelGP(c.X, Y[p], kernel_of(B, f).program)
                row.append(g)
                g.update(lam, c.amp, sig)
                ref = K.Restated(f, c.X, Y[p], lam, c.amp, sig, c.Xs)
                assert ref.cond < 1e6
                if f is NV.flagged:
                    wm, wv, bm, bv = c._expected(ref.mu, ref.var, c.kinds)     # (same K as the case's own: the same cond and tol)
                    assert ref.tol == c.ref.tol
                    poisoned[c.off] = True
                else:
                    wm, wv = ref.mu, NV.clipped(ref.var)
                    bm, bv = np.full(c.M, ref.tol * (1 + np.abs(ref.mu).max())), np.full(c.M, ref.tol * ref.kss.max())
                    assert wv.min() > 1e-5
                mus.append(wm), vars_.append(np.where(poisoned & (f is NV.flagged), 1.0, wv)), bms.append(bm), bvs.append(bv)
            gps.append(row)
            mu, var = np.stack(mus), np.stack(vars_)
            E = O.expected_improvement_lin(coefs, mu, var, BEST_A)
            F = O.feas_prob(mu, var, y_max)
            s0, s1 = np.sqrt(var[0]), np.sqrt(var[1])
            with np.errstate(divide="ignore", invalid="ignore"):
                dE = bms[0] + 0.4 * bvs[0] / (2 * s0)
                dF = np.where(s1 > 0.0, 0.4 * bms[1] / s1 + 0.242 * bvs[1] / (2 * s1 * s1), 0.0)
            acqs.append(E * F)
            bounds.append(dE + np.abs(E) * dF + 8 * EPS * (1 + np.abs(E)))
        want = np.where(poisoned, -np.inf, (acqs[0] + acqs[1]) / 2)
        bound = (bounds[0] + bounds[1]) / 2
        cand = api.Candidates(c.Xs)
        acq, am, mx = api.acq_ei(gps, cand, coefs, y_max, BEST_A)
        _, am2, mx2 = api.acq_ei(gps, cand, coefs, y_max, BEST_A, want_acq=False)
        cand.close()
        fin = ~poisoned
        print(f"[negvar] A acq_ei P=2 S=2: member by member, -Inf at {ints(np.flatnonzero(np.isneginf(acq)))} argmax {am} / {int(np.argmax(want))} "
              f"max|dacq|/bound {(np.abs(acq[fin] - want[fin]) / bound[fin]).max():.3e}")
        assert list(np.flatnonzero(np.isneginf(acq))) == c.off and np.isfinite(acq[fin]).all()
        assert np.all(np.abs(acq[fin] - want[fin]) <= bound[fin])
        assert am == int(np.argmax(want)) and mx == acq[am] and (am2, mx2) == (am, mx)
    finally:
        for row in gps:
            for g in row:
                g.close()


def test_a_only_offenders_compete(B, api):
    """A valid_mask that keeps only offenders: "valid_mask M bytes or NULL: 0 -> acq = 0.0" and "argmax_out / max_out first index of
    the maximum (Julia argmax) over this batch and its value" (bosship.h, boss_acq_ei) — the masked candidates are 0.0, the offenders
    -Inf, so index 0 wins with 0.0.  A batch of offenders alone is -Inf throughout: the first index, -Inf."""
    c = NV.case_a("n130")
    g = fitted_a(B, c)
    mask = np.zeros(c.M, bool)
    mask[c.off] = True
    cand = api.Candidates(c.Xs)
    only = api.Candidates(np.asfortranarray(c.Xs[:, c.off * 3]))
    try:
        acq, am, mx = api.acq_ei([[g]], cand, [1.0], None, BEST_A, valid_mask=mask)
        _, am2, mx2 = api.acq_ei([[g]], cand, [1.0], None, BEST_A, valid_mask=mask, want_acq=False)
        print(f"[negvar] A masked to the offenders: -Inf at {ints(np.flatnonzero(np.isneginf(acq)))} argmax {am} max {mx!r}; want_acq=False ({am2}, {mx2!r})")
        assert list(np.flatnonzero(np.isneginf(acq))) == c.off and np.all(np.delete(acq, c.off) == 0.0)
        assert (am, mx) == (0, 0.0) and (am2, mx2) == (0, 0.0) and mx == acq[am]
        acq, am, mx = api.acq_ei([[g]], only, [1.0], None, BEST_A)
        _, am2, mx2 = api.acq_ei([[g]], only, [1.0], None, BEST_A, want_acq=False)
        print(f"[negvar] A offenders alone: acq {[float(v) for v in acq]} argmax {am} max {mx!r}; want_acq=False ({am2}, {mx2!r})")
        assert np.all(np.isneginf(acq)) and (am, mx) == (0, -np.inf) and (am2, mx2) == (0, -np.inf)
    finally:
        cand.close()
        only.close()


# ------------------------------------------------------------------------------------------ A6: the Python surface
def test_a_python_surface(B, api, O):
    c = NV.case_a("n130")
    pri = dict(lengthscale_priors=[B.MvLogNormal(np.log(c.lam), [0.2, 0.2, 0.2])], amplitude_priors=[B.LogNormal(0.0, 0.2)],
               noise_std_priors=[B.Dirac(c.sig)])
    model = B.HipGaussianProcess(kernel=kernel_of(B, NV.flagged), **pri)
    prm = B.HipGPParams(c.lam[:, None], np.array([c.amp]), np.array([c.sig]))
    data = B.ExperimentData(c.X, c.y[None, :])
    prob = B.BossProblem(None, B.Domain((np.full(3, -1.0), np.full(3, 50.0))), B.ExpectedImprovement(B.LinFitness([1.0])), model, data, None, prm)
    post = model.model_posterior(prm, data)
    try:
        with pytest.raises(api.DomainError) as e:
            post.mean_and_var(c.Xs)
        assert e.value.code == api.BOSS_E_NEG_VAR and e.value.bad_index == c.off[0]
        mu, var = post.mean_and_var(c.Xs_clean)
        assert worst(mu[0], c.want_mu_clean, c.bar_mu_clean) <= 1.0 and worst(var[0], c.want_var_clean, c.bar_var_clean) <= 1.0
    finally:
        post.close()
    best = O.best_so_far([1.0], data.Y, [np.inf])
    want, bound = ei_expected(O, c.want_mu, c.want_var, c.bar_mu, c.bar_var, c.off, best)
    Xs, acq = B.HipBatchAM(points=c.Xs).maximize_acquisition(prob, return_all=True)
    x, val = B.HipBatchAM(points=c.Xs).maximize_acquisition(prob)
    fin = np.setdiff1d(np.arange(c.M), c.off)
    print(f"[negvar] A python surface: DomainError bad_index {e.value.bad_index}; HipBatchAM -Inf at {ints(np.flatnonzero(np.isneginf(acq)))} "
          f"max|dacq|/bound {(np.abs(acq[fin] - want[fin]) / bound[fin]).max():.3e}")
    assert np.array_equal(Xs, c.Xs) and list(np.flatnonzero(np.isneginf(acq))) == c.off
    assert np.all(np.abs(acq[fin] - want[fin]) <= bound[fin])
    j = int(np.argmax(want))
    assert j not in c.off and np.array_equal(x, c.Xs[:, j]) and val == acq[j]


# ------------------------------------------------------------------------------------------ B: boss_gp_predict and its siblings
def check_b(tag, route, api, c, rc, bad, mu, var, cols=None, need_both=True):
    """C1 .. C3 on one call's results, C4 where the call has enough candidates for it; returns the offenders."""
    cols = np.arange(c.M) if cols is None else np.asarray(cols)
    assert not np.isnan(mu).any() and not np.isnan(var).any()
    e_mu, e_var = c.bars(mu, var, cols)
    off = NV.offenders(var)
    print(f"[negvar] B {tag}: route {route} rc {rc} bad_index {bad} offenders {off.size} of {cols.size} (first {ints(off[:4])}) "
          f"|dmu| {e_mu:.3f} |dvar| {e_var:.3f} of their bars (B = {c.B:.3e})")
    NV.contract(api, rc, bad, var)
    assert e_mu <= 1.0 and e_var <= 1.0
    if need_both:
        train = ~c.mid[cols]
        assert off.size and (var[train] >= 0.0).any() and not np.isin(off, np.flatnonzero(~train)).any()
    return off


@pytest.mark.parametrize("N,kernel,M,route", [(40, "matern52", None, "one workgroup"), (40, "sqexp", None, "one workgroup"),
                                              (130, "matern32", None, "G32"), (1030, "matern52", 300, "few-candidates steps / G32")])
def test_b_predict(api, N, kernel, M, route):
    c = NV.case_b(N, kernel)
    g = fitted_b(api, c)
    cols = np.arange(c.M if M is None else M)
    rc, bad, mu, var = NV.predict_raw(api, g, c.Xs[:, cols])
    off = check_b(f"predict N={N} {kernel} M={cols.size}", route, api, c, rc, bad, mu, var, cols)
    if cols.size > 256:                                      # offenders in two blocks of clip_var_kernel, the first not in the last
        assert off[0] < 256 and off[-1] >= 256
    again = NV.predict_raw(api, g, c.Xs[:, cols])
    if not api._acq_counters(g)[0]:                          # (the same path twice; the resident inverses would be another)
        assert again[:2] == (rc, bad) and np.array_equal(again[3], var)


def few_args_calls(api, c, g):
    """Ten boss_gp_predict calls of four training-point candidates each on resident inverse factors (M <= 4: the candidates travel in
    the kernel arguments, host_predict.inc): [(rc, bad_index, mu, var)]."""
    winv_after = int(os.environ.get("BOSS_WINV_AFTER", "2"))
    assert winv_after >= 1 and os.environ.get("BOSS_NO_FEW_ARGS") is None
    g.update(c.lam, c.amp, c.sig)
    for _ in range(winv_after):
        NV.predict_raw(api, g, c.Xs[:, NV.N_MID:NV.N_MID + 4])
    assert api._acq_counters(g)[0] == 1                      # L⁻ᵀ is resident: every call below takes the argument path
    return [NV.predict_raw(api, g, c.Xs[:, NV.N_MID + 4 * k:NV.N_MID + 4 * k + 4]) for k in range(10)]


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
entry.build()
from boss_jl_amd import api
import neg_var_cases as NV
import test_gpu_neg_var as T
c = NV.case_b(1030, "matern52")
res = T.few_args_calls(api, c, T.fitted_b(api, c))
print("RES " + json.dumps([[rc, bad, [v.hex() for v in mu], [v.hex() for v in var]] for rc, bad, mu, var in res]))
"""


def test_b_argument_path_fused_and_three_launch(api):
    """M <= 4 on N = 1030 behind BOSS_WINV_AFTER calls: winv_args_kernel's last-workgroup reduction here, and winv_finish_host_kernel
    in one fresh child process with BOSS_FEW_FUSED=0 (the knob is read once per process).  Ten calls on consecutive groups of four
    training points, C1 .. C3 each.  Over the ten at least one call fails and at least one succeeds: a training-point candidate
    offends with probability about 0.3 (float64 restatement: 22 to 43 % per case, MI355X: 23 to 32 %), so a call of four succeeds
    with 0.7⁴ = 0.24; all ten failing has a chance of 0.76¹⁰ = 0.06 and all ten succeeding one of 6e-7 — on a given build the outcome
    is fixed by the summation order (MI355X: 8 fail, 2 succeed).
    DESIGN.md §4.3: the last workgroup "reduces the per-workgroup partials in the fixed order of the multi-launch path:
    bit-identical" — so the two forms must return the same arrays, offenders included."""
    c = NV.case_b(1030, "matern52")
    g = fitted_b(api, c)
    res = few_args_calls(api, c, g)
    fails = 0
    for k, (rc, bad, mu, var) in enumerate(res):
        cols = np.arange(NV.N_MID + 4 * k, NV.N_MID + 4 * k + 4)
        check_b(f"predict N=1030 M=4 group {k}", "winv_args_kernel", api, c, rc, bad, mu, var, cols, need_both=False)
        fails += rc == api.BOSS_E_NEG_VAR
    assert 0 < fails < 10, fails
    # M = 1, 2, 3: the other instantiations of the kernel
    for M in (1, 2, 3):
        cols = np.arange(NV.N_MID, NV.N_MID + 12).reshape(-1, M)
        for k, cs in enumerate(cols):
            rc, bad, mu, var = NV.predict_raw(api, g, c.Xs[:, cs])
            check_b(f"predict N=1030 M={M} group {k}", "winv_args_kernel", api, c, rc, bad, mu, var, cs, need_both=False)
    code = CHILD % {"root": ROOT, "tests": HERE}
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], env=dict(os.environ, BOSS_FEW_FUSED="0"),
                       capture_output=True, text=True, timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RES ")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-3000:] + r.stderr[-3000:]
    child = json.loads(lines[0][4:])
    for k, ((rc, bad, mu, var), (rc_c, bad_c, mu_c, var_c)) in enumerate(zip(res, child)):
        mu_c, var_c = np.array([float.fromhex(v) for v in mu_c]), np.array([float.fromhex(v) for v in var_c])
        cols = np.arange(NV.N_MID + 4 * k, NV.N_MID + 4 * k + 4)
        check_b(f"predict N=1030 M=4 group {k}, BOSS_FEW_FUSED=0", "winv_finish_host_kernel", api, c, rc_c, bad_c, mu_c, var_c, cols, need_both=False)
        assert (rc_c, bad_c) == (rc, bad) and np.array_equal(mu_c, mu) and np.array_equal(var_c, var)


@pytest.mark.parametrize("N,kernel", [(40, "matern52"), (130, "matern52")])
def test_b_predict_grad(api, N, kernel):
    c = NV.case_b(N, kernel)
    g = fitted_b(api, c)
    rc, bad, mu, var, dmu, dvar = NV.predict_grad_raw(api, g, c.Xs)
    check_b(f"predict_grad N={N} {kernel}", "one workgroup" if N <= 128 else "G32 + adjoint", api, c, rc, bad, mu, var)
    assert not np.isnan(dmu).any() and not np.isnan(dvar).any()


def test_b_predict_cov(api):
    c = NV.case_b(130, "matern52")
    g = fitted_b(api, c)
    rc, bad, mu, cov = NV.predict_cov_raw(api, g, c.Xs)
    check_b("predict_cov N=130 (the diagonal)", "predict_cov_kernel + clip_cov_diag_kernel", api, c, rc, bad, mu, np.diag(cov).copy())
    assert not np.isnan(cov).any() and np.array_equal(cov, cov.T)


# ------------------------------------------------------------------------------------------ B: the acquisition calls
def check_b_acq(tag, route, c, acq, am, mx, best, grad=None):
    """-Inf only at training-point candidates, and at one at least; no NaN; the arg-max is a midpoint and np.argmax(acq); the gradient
    columns of -Inf candidates are exactly 0.  The midpoints (σ² >= 1e9, far from every clip) are held to the restatement:
    |ΔEI| <= Δμ + 0.4·Δσ²/(2σ) with C3's bars, plus 8·2⁻⁵²(1 + EI) for the epilogue's own roundings."""
    inf = np.isneginf(acq)
    mid = c.mid[:acq.size]
    assert not np.isnan(acq).any() and inf.any() and not inf[mid].any() and np.isfinite(acq[~inf]).all()
    if am is not None:
        assert am == int(np.argmax(acq)) and mid[am] and mx == acq[am]
    from oracle import gp_oracle as O
    mu, var = c.ref.mu[:acq.size][mid], c.ref.var[:acq.size][mid]
    want = O.expected_improvement_lin([1.0], mu[None, :], var[None, :], best)
    bound = c.B * (1 + np.abs(c.ref.mu).max()) + 0.4 * c.B * c.a2 / (2 * np.sqrt(var)) + 8 * EPS * (1 + np.abs(want))
    ratio = float((np.abs(acq[mid] - want) / bound).max())
    line = f"[negvar] B {tag}: route {route} -Inf at {int(inf.sum())} of {acq.size} (first {ints(np.flatnonzero(inf)[:4])}) argmax {am} max {mx!r} midpoint |dEI| {ratio:.3f} of its bound"
    if grad is not None:
        assert not np.isnan(grad).any() and np.all(grad[:, inf] == 0.0) and np.any(grad[:, mid] != 0.0)
        line += f"; gradient columns at -Inf all zero, largest elsewhere {np.abs(grad[:, ~inf]).max():.3e}"
    print(line)
    assert ratio <= 1.0
    return inf


@pytest.mark.parametrize("N", [130, 1030])
def test_b_acq_ei(api, N):
    c = NV.case_b(N, "matern52")
    g = fitted_b(api, c)
    best = float(c.y.max())
    cand = api.Candidates(c.Xs)
    try:
        acq, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, want_acq=True)
    finally:
        cand.close()
    check_b_acq(f"acq_ei N={N}", f"full kernel, path {api._acq_path(0)[0]}", c, acq, am, mx, best)


@pytest.mark.parametrize("N", [40, 130])
def test_b_acq_ei_grad(api, N):
    c = NV.case_b(N, "matern52")
    g = fitted_b(api, c)
    best = float(c.y.max())
    acq, dacq = api.acq_ei_grad([g], c.Xs, [1.0], None, best)
    check_b_acq(f"acq_ei_grad N={N}", "ei_grad_kernel", c, acq, None, None, best, dacq)


def test_b_acq_ei_mc_with_an_identity_fitness(B, api):
    """boss_acq_ei_mc under the fitness y -> y: mean over ε of max(0, μ + σε − best), -Inf where the variance offends (fitness.hpp)."""
    c = NV.case_b(130, "matern52")
    g = fitted_b(api, c)
    best = float(c.y.max())
    fit = B.DeviceFitness(lambda yv: yv[0], 1).program
    eps = np.random.default_rng(5).standard_normal((1, 64))
    cand = api.Candidates(c.Xs)
    try:
        acq, am, mx = api.acq_ei_mc([[g]], cand, fit, eps, None, best)
        _, am2, mx2 = api.acq_ei_mc([[g]], cand, fit, eps, None, best, want_acq=False)
    finally:
        cand.close()
    inf, mid = np.isneginf(acq), c.mid
    print(f"[negvar] B acq_ei_mc N=130: route MC epilogue, -Inf at {int(inf.sum())} of {c.M} (first {ints(np.flatnonzero(inf)[:4])}) argmax {am} max {mx!r}")
    assert not np.isnan(acq).any() and inf.any() and not inf[mid].any() and np.isfinite(acq[~inf]).all() and np.all(acq[~inf] >= 0.0)
    assert am == int(np.argmax(acq)) and mid[am] and mx == acq[am] and (am2, mx2) == (am, mx)
    # the midpoints against the same Monte-Carlo mean on the restated moments: Lipschitz 1 in μ and |ε| in σ
    mu, sd = c.ref.mu[mid], np.sqrt(c.ref.var[mid])
    want = np.maximum(0.0, mu[:, None] + sd[:, None] * eps[0][None, :] - best).mean(1)
    bound = c.B * (1 + np.abs(c.ref.mu).max()) + np.abs(eps).mean() * c.B * c.a2 / (2 * sd) + 64 * EPS * (1 + np.abs(want))
    assert np.all(np.abs(acq[mid] - want) <= bound), float((np.abs(acq[mid] - want) / bound).max())


@pytest.mark.parametrize("N,fused", [(130, False), (1030, True)])
def test_b_update_acq(api, N, fused):
    """boss_gp_update_acq: "mu_out / var_out M posterior moments (unclipped: what mean_and_var returns before _clip_var; the EI epilogue
    clips)" (bosship.h) — one call returns both, so its -Inf candidates are exactly those whose returned variance is below -1e-8.
    N = 130 runs the two phases one after the other (acq_epilogue_kernel); N = 1030, three or more block columns, lets the
    substitution ride along the factorisation (rider_final_kernel's epilogue), as tests/test_gpu_rider.py asserts for such shapes."""
    c = NV.case_b(N, "matern52")
    g = api.GP(c.X, c.y, c.kernel)
    best = float(c.y.max())
    cand = api.Candidates(c.Xs)
    try:
        r = g.update_acq(c.lam, c.amp, c.sig, cand, 1.0, None, best, want_acq=True, want_moments=True)
        r2 = g.update_acq(c.lam, c.amp, c.sig, cand, 1.0, None, best, want_acq=False)
    finally:
        cand.close()
        g.close()
    assert r["fused"] == fused and r2["fused"] == fused
    inf = check_b_acq(f"update_acq N={N}", f"fused {r['fused']}", c, r["acq"], r["argmax"], r["max"], best)
    e_mu, e_var = c.bars(r["mu"], r["var"])
    print(f"[negvar] B update_acq N={N}: |dmu| {e_mu:.3f} |dvar| {e_var:.3f} of their bars, variances in the band {int(((r['var'] < 0) & (r['var'] >= -1e-8)).sum())}")
    assert e_mu <= 1.0 and e_var <= 1.0 and abs(r["logpdf"] - c.ref.logpdf) <= c.B * (1 + abs(c.ref.logpdf))
    assert np.array_equal(np.flatnonzero(inf), NV.offenders(r["var"]))
    assert (r2["argmax"], r2["max"]) == (r["argmax"], r["max"])


def test_b_arg_max_only_path(api):
    """N = 1030, M = 37 + 1030 under the lowered thresholds of tests/test_gpu_acq_prune.py: the pruned call reports PRUNED and finds
    the full kernel's arg-max (that file's same()); then with a valid_mask that removes every midpoint, so that only near-zero-variance
    and -Inf candidates (and the masked 0.0) compete."""
    from test_gpu_acq_prune import same
    c = NV.case_b(1030, "matern52")
    g = fitted_b(api, c)
    best = float(c.y.max())
    cand = api.Candidates(c.Xs)
    api._acq_prune_set(0, min_tiles=0, K=64, s=2, cap=1024, slack=1.0)
    try:
        for tag, mask in (("all candidates", None), ("midpoints masked", ~c.mid)):
            _, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, valid_mask=mask, want_acq=False)
            rep = api._acq_path(0)
            acq, am_f, mx_f = api.acq_ei([[g]], cand, [1.0], None, best, valid_mask=mask, want_acq=True)
            inf = np.isneginf(acq)
            print(f"[negvar] B arg-max-only, {tag}: path {rep} pruned ({am}, {mx!r}) full ({am_f}, {mx_f!r}) -Inf at {int(inf.sum())} of {c.M} "
                  f"|max - acq[argmax]| {abs(mx - acq[am_f]):.3e}")
            assert rep[0] == PRUNED, rep
            assert inf.any() and not inf[c.mid].any() and not np.isnan(acq).any()
            same((am, mx), (acq, am_f, mx_f))
            assert not inf[am] and am_f == int(np.argmax(acq))
            if mask is None:
                assert c.mid[am]
            else:
                assert np.all(acq[c.mid] == 0.0)
    finally:
        api._acq_prune_set(0, min_tiles=-2, K=-2, s=-2, cap=-2, slack=1.0)
        cand.close()


# ------------------------------------------------------------------------------------------ B: the one-call warp paths
def test_b_one_call_warp_paths(B, api):
    """Identity input program, P = S = 1, N = 130.  bosship.h on the one-call paths: "What the calls return, bit for bit: with an input
    program alone, boss_acq_ei_warp what boss_acq_ei returns on a candidate set created from boss_warp_apply's X_out,
    boss_warp_predict what boss_gp_predict returns there; at S = 1, boss_warp_predict_grad what boss_warp_apply ->
    boss_gp_predict_grad per output -> boss_warp_moments return, and boss_acq_ei_grad_warp what boss_acq_ei_grad_moments makes of
    that", and on the moments stage: "out_prog == NULL passes mu_ and var_ through bit for bit" — so each one-call path must show
    the offenders of its plain twin."""
    c = NV.case_b(130, "matern52")
    g = fitted_b(api, c)
    best = float(c.y.max())
    warp = api.WarpProgram(B.trace_mean(lambda x: [x[0]], 1, 0, 1), 1, None)
    cand = None
    try:
        X_out, _ = warp.apply(c.Xs)
        assert np.array_equal(X_out, c.Xs)
        cand = api.Candidates(X_out)
        plain = NV.predict_raw(api, g, X_out)
        rc, bad, mu, var = NV.warp_predict_raw(api, warp, g, c.Xs)
        check_b("warp_predict N=130", "warp_call, member by member", api, c, rc, bad, mu, var)
        assert (rc, bad) == plain[:2] and np.array_equal(mu, plain[2]) and np.array_equal(var, plain[3])
        plain_g = NV.predict_grad_raw(api, g, X_out)
        rc, bad, mu, var, dmu, dvar = NV.warp_predict_raw(api, warp, g, c.Xs, grad=True)
        off_g = check_b("warp_predict_grad N=130", "warp_call, member by member", api, c, rc, bad, mu, var)
        assert (rc, bad) == plain_g[:2] and np.array_equal(var, plain_g[3]) and np.array_equal(mu, plain_g[2])
        acq_p, am_p, mx_p = api.acq_ei([[g]], cand, [1.0], None, best)
        acq, am, mx = warp.acq_ei([[g]], c.Xs, [1.0], None, best)
        check_b_acq("acq_ei_warp N=130", "warp_call + acq_epilogue_kernel", c, acq, am, mx, best)
        assert np.array_equal(acq, acq_p) and (am, mx) == (am_p, mx_p)
        acq, dacq = warp.acq_ei_grad([[g]], c.Xs, [1.0], None, best)
        inf = check_b_acq("acq_ei_grad_warp N=130", "warp_call + ei_grad_kernel", c, acq, None, None, best, dacq)
        assert np.array_equal(np.flatnonzero(inf), off_g)
    finally:
        if cand is not None:
            cand.close()
        warp.close()
