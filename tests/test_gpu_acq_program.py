"""Acquisition programs on the device (pytest -m gpu): boss_acq_prog, boss_acq_prog_moments, boss_acq_prog_grad,
boss_acq_prog_grad_moments and the plugin level on top of them (B.DeviceAcquisition with HipBatchAM, HipGradientAM,
HipSequentialBatchAM, bo()).

Shapes: N = 130, d = 3 (two block columns), M in {1, 63, 65, 257}, S in {1, 3}, P in {1, 2, 3}, Q in {0, 1, 4}.  Bars:
  fixture pins         device_C·u·cond of tests/acq_tails_cases.py, on the groups tests/acq_program_cases.py selects;
  against boss_acq_ei  2·device_C·u·cond, cond from the fp64 restatement of acq_truth's condition sum at the predicted moments — each
                       side is within device_C·u·cond of the truth at those moments;
  against the host interpreter   8u(|cᵀμ| + β·σ_f) for UCB (three roundings and a square root), 8u·Σσ² for the variance sum;
  finite differences   h = 1e-5, 1e-6·max(1, |∂|): the rule DeviceKernel(grad=True) is held to;
everything else is bit for bit."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acq_tails_cases as T  # noqa: E402
import neg_var_cases as NV  # noqa: E402

pytestmark = pytest.mark.gpu
U = T.U
N_, D_ = 130, 3
MS = (1, 63, 65, 257)
INF = np.inf


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd
    boss_jl_amd.api.load_library()
    assert boss_jl_amd.api.device_count() >= 1
    return boss_jl_amd


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


@pytest.fixture(scope="module")
def cases(B):
    import acq_program_cases
    return acq_program_cases


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------ shared handles (fitted once, never changed)
def sqexp(u, v):
    return np.exp(-0.5 * sum((u[k] - v[k]) ** 2 for k in range(len(u))))


# ∂Y_p/∂x of the three outputs of World (the gradient observations are those of the observed functions)
DY = [lambda X: 3 * np.cos(3 * X),
      lambda X: np.stack([np.ones(X.shape[1]), -np.ones(X.shape[1]), -0.8 * np.sin(4 * X[2])]),
      lambda X: np.stack([-2 * np.sin(2 * X[0]) * X[2], np.zeros(X.shape[1]), np.cos(2 * X[0])])]


class World:
    """3 samples × 3 outputs of every handle kind on N = 130, d = 3: gps[kind][s][p]."""

    def __init__(self, B):
        api = B.api
        rng = np.random.default_rng(42)
        self.X = X = rng.uniform(0, 1, (D_, N_))
        Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1] + 0.2 * np.cos(4 * X[2]), np.cos(2 * X[0]) * X[2]])
        self.Y = Y
        lam = rng.uniform(0.35, 0.8, (3, D_, 3))                 # [p][:, s]
        amp = rng.uniform(0.8, 1.5, (3, 3))
        sig = rng.uniform(0.04, 0.1, (3, 3))
        self.kprog = B.DeviceKernel(sqexp, D_, grad=True).program
        self.gps = {k: [[None] * 3 for _ in range(3)] for k in ("plain", "kprog", "gradobs", "set")}
        n = 33                                                   # gradient observations: n (1 + d) = 132 rows
        Xg = X[:, :n]
        for p in range(3):
            members, _, st = api.fit_batch(X, Y[p], "matern52", lam[p], amp[p], sig[p])
            assert list(st) == [0, 0, 0]
            for s in range(3):
                g = api.GP(X, Y[p], "matern52")
                g.update(lam[p][:, s], amp[p, s], sig[p, s])
                k = api.KernelGP(X, Y[p], self.kprog, grad=True)
                k.update(lam[p][:, s], amp[p, s], sig[p, s])
                dY = DY[p](Xg)
                gg = api.GradGP(Xg, Y[p][:n], dY, "sqexp")
                gg.update(lam[p][:, s], amp[p, s], sig[p, s], 0.1)
                self.gps["plain"][s][p], self.gps["kprog"][s][p], self.gps["gradobs"][s][p], self.gps["set"][s][p] = g, k, gg, members[s]
        self.Xs = {M: np.asfortranarray(np.random.default_rng(100 + M).uniform(0.03, 0.97, (D_, M))) for M in MS}
        self.best = {P: float(np.median(np.array(COEFS[P]) @ Y[:P])) for P in (1, 2, 3)}     # (candidates on both sides of z = 0)

    def rows(self, kind, S, P):
        return [[self.gps[kind][s][p] for p in range(P)] for s in range(S)]

    def moments(self, kind, S, P, Xs, grad=False):
        """predict (or predict_grad) of every member: arrays [S][P][M] (and [S][P][d][M])."""
        out = [[(g.predict_grad(Xs) if grad else g.predict(Xs)) for g in row] for row in self.rows(kind, S, P)]
        return tuple(np.stack([np.stack([r[k] for r in row]) for row in out]) for k in range(4 if grad else 2))


COEFS = {1: [1.0], 2: [1.0, -0.5], 3: [0.7, 0.2, -1.1]}
YMAX = {1: [INF], 2: [INF, 0.6], 3: [1.5, INF, 0.4]}
_world = {}


@pytest.fixture(scope="module")
def W(B):
    if "w" not in _world:
        _world["w"] = World(B)
    return _world["w"]


# ------------------------------------------------------------------------------------------ 1. fixture pins on the device
def test_values_on_the_fixture(api, cases):
    C = T.load()["header"]["device_C"]["value"]
    worst = 0.0
    for g in cases.value_groups():
        prog, q = cases.group_program(g)
        acq, am, mx = api.acq_prog_moments(g["mu"], g["var"], prog, q)
        r = T.ratio(acq, g["truth"], g["cond"])
        worst = max(worst, r)
        bad = T.misses(acq, g["truth"], g["cond"], C)
        assert not bad.any(), (g["name"], np.flatnonzero(bad)[:5], r)
        assert mx == acq[am] and am == int(np.argmax(acq))
    print(f"device, values: worst err/(u·cond) {worst:.3g} against C = {C} over {len(cases.value_groups())} groups")


def test_gradients_on_the_fixture(api, cases):
    hdr = T.load()["header"]["device_C"]
    for g in cases.grad_groups():
        prog, q = cases.group_program(g)
        acq, dacq = api.acq_prog_grad_moments(g["mu"], g["var"], g["dmu"][None], g["dvar"][None], prog, q)
        print(f"device, {g['name']}: value {T.ratio(acq, g['truth'], g['cond']):.3g} gradient {T.ratio(dacq, g['gtruth'], g['gcond']):.3g} "
              f"against C = {hdr['grad']}")
        assert not T.misses(acq, g["truth"], g["cond"], hdr["value"]).any(), g["name"]
        assert not T.misses(dacq, g["gtruth"], g["gcond"], hdr["grad"]).any(), g["name"]


def test_scaled_variances_miss_the_bar(api, cases):
    """The teeth of tests/test_gpu_acq_tails.py on the program path: variances off by a factor 1 + 2⁻⁴⁰ against the unscaled truths."""
    C = T.load()["header"]["device_C"]["value"]
    scale = 1.0 + 2.0 ** -40
    seen = 0
    for g in cases.value_groups():
        if not g["name"].startswith("tail-"):
            continue
        prog, q = cases.group_program(g)
        acq, _, _ = api.acq_prog_moments(g["mu"], g["var"] * scale, prog, q)
        bad = T.misses(acq, g["truth"], g["cond"], C)
        print(f"{g['name']}: variances × (1 + 2⁻⁴⁰): {int(bad.sum())} of {g['M']} outside the bar")
        if g["best"] == 0.0:
            seen += 1
            assert bad.sum() >= 10, f"{g['name']}: a relative error of 2⁻⁴⁰ in σ² passes the bar"
    assert seen == 6


# ------------------------------------------------------------------------------------------ 2. agreement with the built-in EI
@pytest.mark.parametrize("kind", ["plain", "kprog", "gradobs", "set"])
def test_ei_spelled_as_a_program_agrees_with_boss_acq_ei(api, O, cases, W, kind):
    C = T.load()["header"]["device_C"]["value"]
    for P in (1, 2, 3):
        prog = api_program(cases, P)
        q = cases.ei_fp_q(P, W.best[P], YMAX[P])
        for S in (1, 3):
            for M in MS:
                Xs = W.Xs[M]
                cand = api.Candidates(Xs)
                try:
                    got, am, mx = api.acq_prog(W.rows(kind, S, P), cand, prog, q)
                    want, am_w, mx_w = api.acq_ei(W.rows(kind, S, P), cand, COEFS[P], YMAX[P], W.best[P])
                finally:
                    cand.close()
                mu, var = W.moments(kind, S, P, Xs)
                assert np.all(var > 0)
                conds = np.stack([cases.ei_fp_cond(O, COEFS[P], mu[s], var[s], W.best[P], YMAX[P]) for s in range(S)])
                cond = conds[0] if S == 1 else T.mean_cond(conds, np.stack([want] * S))
                bar = 2 * C * U * cond
                tiny = want < 1e-280                         # (products in or next to the denormals: the fixture's "tiny" rule)
                assert T.check_tiny(got[tiny])
                assert np.all(np.abs(got - want)[~tiny] <= bar[~tiny]), (kind, P, S, M, float(np.max(np.abs(got - want)[~tiny] / bar[~tiny])))
                assert mx == got[am] and am == int(np.argmax(got))
                top = np.sort(want)[::-1]
                if M == 1 or top[0] - top[1] > 2 * bar.max():
                    assert am == am_w, (kind, P, S, M)


_ei_programs = {}


def api_program(cases, P):
    if P not in _ei_programs:
        import boss_jl_amd as B
        _ei_programs[P] = B.trace_acquisition(cases.ei_fp(COEFS[P]), P, 1 + P)
    return _ei_programs[P]


# ------------------------------------------------------------------------------------------ 3. handle path == moments path, bit for bit
PROGRAMS_BY_PQ = {(1, 0): "ucb1", (2, 0): "ucb", (3, 0): "max_variance", (2, 1): "clamp", (3, 4): "pi", (1, 2): "ei_fp1"}


def q_of(Q):
    return np.array([0.4, 1.5, INF, 0.3][:Q])


@pytest.mark.parametrize("kind", ["plain", "kprog", "gradobs", "set"])
def test_handle_path_equals_moments_path(api, cases, W, kind):
    for (P, Q), name in PROGRAMS_BY_PQ.items():
        prog, q = cases.programs()[name], q_of(Q)
        for S in (1, 3):
            for M in MS:
                Xs = W.Xs[M]
                mask = np.arange(M) % 7 != 3 if M > 1 else None
                cand = api.Candidates(Xs)
                try:
                    a1, am1, mx1 = api.acq_prog(W.rows(kind, S, P), cand, prog, q, mask)
                    a2, am2, mx2 = api.acq_prog(W.rows(kind, S, P), cand, prog, q, mask)
                    _, am3, mx3 = api.acq_prog(W.rows(kind, S, P), cand, prog, q, mask, want_acq=False)
                finally:
                    cand.close()
                mu, var = W.moments(kind, S, P, Xs)
                a4, am4, mx4 = api.acq_prog_moments(mu, var, prog, q, mask)
                what = (kind, name, S, M)
                assert same_bits(a1, a2) and (am1, mx1) == (am2, mx2) == (am3, mx3), what
                assert same_bits(a1, a4) and am1 == am4 and mx1 == mx4, what
                if mask is not None:
                    assert np.all(np.isneginf(a1[~mask]))


@pytest.mark.parametrize("kind", ["plain", "kprog", "gradobs", "set"])
def test_gradient_handle_path_equals_moments_path(api, cases, W, kind):
    for name in ("ucb", "pi", "ei_fp1", "long_minmax", "clamp"):
        _, P, Q = cases.CLOSURES[name]
        prog, q = cases.programs()[name], q_of(Q)
        for S in (1, 3):
            for M in (1, 65, 257):
                Xs = W.Xs[M]
                mask = np.arange(M) % 5 != 2 if M > 1 else None
                a1, g1 = api.acq_prog_grad(W.rows(kind, S, P), Xs, prog, q, mask, 0.0)
                a2, g2 = api.acq_prog_grad(W.rows(kind, S, P), Xs, prog, q, mask, 0.0)
                mu, var, dmu, dvar = W.moments(kind, S, P, Xs, grad=True)
                a3, g3 = api.acq_prog_grad_moments(mu, var, dmu, dvar, prog, q, mask, 0.0)
                what = (kind, name, S, M)
                assert same_bits(a1, a2) and same_bits(g1, g2), what
                assert same_bits(a1, a3) and same_bits(g1, g3), what
                if mask is not None:
                    assert np.all(a1[~mask] == 0.0) and np.all(g1[:, ~mask] == 0.0)
                # and the value of the gradient call is the value call's, to the last bit of the sample sum
                cand = api.Candidates(Xs)
                try:
                    a4, _, _ = api.acq_prog(W.rows(kind, S, P), cand, prog, q, mask, 0.0)
                finally:
                    cand.close()
                assert same_bits(a1, a4), what


# ------------------------------------------------------------------------------------------ 4. against the host interpreter
@pytest.mark.parametrize("kind", ["plain", "kprog", "gradobs", "set"])
def test_ucb_and_variance_sum_against_the_host_interpreter(api, cases, W, kind):
    c, beta = np.array([1.0, -0.5]), 2.0
    for M in MS:
        Xs = W.Xs[M]
        cand = api.Candidates(Xs)
        try:
            ucb, _, _ = api.acq_prog(W.rows(kind, 1, 2), cand, cases.programs()["ucb"])
            mv, _, _ = api.acq_prog(W.rows(kind, 1, 3), cand, cases.programs()["max_variance"])
        finally:
            cand.close()
        mu, var = W.moments(kind, 1, 3, Xs)
        want = cases.programs()["ucb"].eval_host(mu[0, :2], var[0, :2])
        bar = 8 * U * (np.abs(c @ mu[0, :2]) + beta * np.sqrt((c * c) @ var[0, :2]))
        assert np.all(np.abs(ucb - want) <= bar), (kind, M, float(np.max(np.abs(ucb - want) / bar)))
        want = cases.programs()["max_variance"].eval_host(mu[0], var[0])
        assert np.all(np.abs(mv - want) <= 8 * U * var[0].sum(0)), (kind, M)


# ------------------------------------------------------------------------------------------ 5. conventions
def test_variance_conventions_on_moments(api, cases):
    rng = np.random.default_rng(3)
    P, M, d = 2, 65, 3
    prog = cases.programs()["ucb"]
    mu, var = rng.standard_normal((1, P, M)), rng.uniform(0.1, 2.0, (1, P, M))
    dmu, dvar = rng.standard_normal((1, P, d, M)), rng.standard_normal((1, P, d, M))
    band, zero, poisoned = var.copy(), var.copy(), var.copy()
    band[0, 1, 7], zero[0, 1, 7] = -1e-9, 0.0
    band[0, 0, 64], zero[0, 0, 64] = -1e-8, 0.0
    poisoned[0, 1, 7], poisoned[0, 0, 33] = -1e-7, -1.0000001e-8
    a_b, am_b, mx_b = api.acq_prog_moments(mu, band, prog)
    a_z, am_z, mx_z = api.acq_prog_moments(mu, zero, prog)
    assert same_bits(a_b, a_z) and (am_b, mx_b) == (am_z, mx_z) and np.all(np.isfinite(a_b))
    g_b, g_z = api.acq_prog_grad_moments(mu, band, dmu, dvar, prog), api.acq_prog_grad_moments(mu, zero, dmu, dvar, prog)
    assert same_bits(g_b[0], g_z[0]) and same_bits(g_b[1], g_z[1]) and same_bits(g_b[0], a_b)
    # a clipped variance contributes no σ² term: the gradient there is ā_μ ∂μ alone (UCB: c_p), the other output's terms unchanged
    c = np.array([1.0, -0.5])
    _, dm, dv = prog.eval_host(mu[0], zero[0], want_grad=True)
    terms = [dm[0, 7] * dmu[0, 0, :, 7], dv[0, 7] * dvar[0, 0, :, 7], dm[1, 7] * dmu[0, 1, :, 7]]
    assert np.all(np.abs(g_b[1][:, 7] - (terms[0] + terms[1] + terms[2])) <= 8 * U * sum(np.abs(t) for t in terms))
    assert np.array_equal(dm[:, 7], c)
    a_p, am_p, mx_p = api.acq_prog_moments(mu, poisoned, prog)
    a_c, _, _ = api.acq_prog_moments(mu, var, prog)
    bad = np.zeros(M, bool)
    bad[[7, 33]] = True
    assert np.all(np.isneginf(a_p[bad])) and same_bits(a_p[~bad], a_c[~bad]) and am_p == int(np.argmax(a_p)) and not bad[am_p]
    ga_p, g_p = api.acq_prog_grad_moments(mu, poisoned, dmu, dvar, prog)
    ga_c, g_c = api.acq_prog_grad_moments(mu, var, dmu, dvar, prog)
    assert same_bits(ga_p, a_p) and np.all(g_p[:, bad] == 0.0) and same_bits(g_p[:, ~bad], g_c[:, ~bad])
    # S = 3 with one poisoned sample: the mean is -Inf, its gradient 0
    mu3, var3 = np.concatenate([mu, mu + 0.1, mu - 0.1]), np.concatenate([var, poisoned, var])
    a3, _, _ = api.acq_prog_moments(mu3, var3, prog)
    ga3, g3 = api.acq_prog_grad_moments(mu3, var3, np.concatenate([dmu] * 3), np.concatenate([dvar] * 3), prog)
    assert np.all(np.isneginf(a3[bad])) and np.all(np.isfinite(a3[~bad])) and same_bits(a3, ga3) and np.all(g3[:, bad] == 0.0)


def test_variance_conventions_on_a_posterior(B, api, cases):
    """Construction A of tests/neg_var_cases.py (N = 130, 70 candidates): far candidates whose variance the flagged kernel puts at
    -0.99e-8 and -5e-9 (clipped: UCB = μ + β·0 = 0 exactly), at -2e-8 and a wide offender (-Inf), the healthy ones untouched."""
    c = NV.case_a("n130")
    g = api.KernelGP(c.X, c.y, B.DeviceKernel(NV.flagged, 3, grad=True).program, grad=True)
    try:
        g.update(c.lam, c.amp, c.sig)
        prog = cases.programs()["ucb1"]
        got = {}
        for name, Xs in (("poisoned", c.Xs), ("clean", c.Xs_clean)):
            cand = api.Candidates(Xs)
            try:
                got[name] = api.acq_prog([[g]], cand, prog)
            finally:
                cand.close()
        acq, am, mx = got["poisoned"]
        clean = got["clean"][0]
        off = np.zeros(c.M, bool)
        off[c.off] = True
        clip = np.flatnonzero(c.far & (c.want_var == 0.0))
        assert list(np.flatnonzero(np.isneginf(acq))) == c.off and len(clip) >= 2
        assert np.all(acq[clip] == 0.0) and same_bits(acq[~off], clean[~off])
        assert not off[am] and am == int(np.argmax(acq)) and mx == acq[am]
        a, dg = api.acq_prog_grad([[g]], c.Xs, prog)
        assert same_bits(a, acq) and np.all(dg[:, off] == 0.0) and np.all(np.isfinite(dg))
    finally:
        g.close()


def test_mask_argmax_nan_and_ties(B, api, cases):
    rng = np.random.default_rng(9)
    P, M, d = 2, 257, 3
    prog = cases.programs()["ucb"]
    mu, var = rng.standard_normal((3, P, M)), rng.uniform(0.1, 2.0, (3, P, M))
    dmu, dvar = rng.standard_normal((3, P, d, M)), rng.standard_normal((3, P, d, M))
    free, _, _ = api.acq_prog_moments(mu, var, prog)
    mask = np.ones(M, bool)
    mask[[0, 100, 256, int(np.argmax(free))]] = False
    for outside in (-INF, 0.0, -7.5):
        a, am, mx = api.acq_prog_moments(mu, var, prog, None, mask, outside)
        assert np.all(a[~mask] == outside) and same_bits(a[mask], free[mask])
        want_am = int(np.argmax(a))
        assert am == want_am and mx == a[am]
        ga, g = api.acq_prog_grad_moments(mu, var, dmu, dvar, prog, None, mask, outside)
        assert same_bits(ga, a) and np.all(g[:, ~mask] == 0.0) and np.all(g[:, mask] != 0.0)
    # default: -Inf
    assert np.all(np.isneginf(api.acq_prog_moments(mu, var, prog, None, mask)[0][~mask]))
    # everything masked: the first index
    for outside in (-INF, 0.0):
        a, am, mx = api.acq_prog_moments(mu, var, prog, None, np.zeros(M, bool), outside)
        assert np.all(a == outside) and am == 0 and mx == outside
    # NaN from the program wins the arg-max (first NaN)
    lg = B.trace_acquisition(lambda mu, var, q: np.log(mu[0]) + var[0], 1, 0)
    m1 = np.abs(mu[:1, :1]) + 0.5
    m1[0, 0, 200], m1[0, 0, 230] = -1.0, -2.0
    a, am, mx = api.acq_prog_moments(m1, var[:1, :1], lg)
    assert np.isnan(a[200]) and np.isnan(a[230]) and np.isfinite(np.delete(a, [200, 230])).all() and am == 200 and np.isnan(mx)
    # ties go to the first index: M = 2049 candidates spread over the epilogue's 1024 threads
    M = 2049
    mv = cases.programs()["max_variance"]
    mu_t, var_t = np.zeros((1, 3, M)), np.full((1, 3, M), 0.25)
    a, am, mx = api.acq_prog_moments(mu_t, var_t, mv)
    assert np.all(a == 0.75) and am == 0 and mx == 0.75
    var_t[0, 1, [1500, 2048, 1030]] = 0.5
    a, am, mx = api.acq_prog_moments(mu_t, var_t, mv)
    assert am == 1030 and mx == 1.0
    var_t[0, 1, 1030] = 0.25
    assert api.acq_prog_moments(mu_t, var_t, mv)[1] == 1500


# ------------------------------------------------------------------------------------------ 6. sample sums
@pytest.mark.parametrize("kind", ["moments", "plain", "kprog", "gradobs", "set"])
def test_three_samples_are_the_ordered_sum_of_single_sample_calls(api, cases, W, kind):
    for name in ("ucb", "pi", "long_minmax"):
        _, P, Q = cases.CLOSURES[name]
        prog, q = cases.programs()[name], q_of(Q)
        for M in (63, 257):
            Xs = W.Xs[M]
            if kind == "moments":
                mu, var, dmu, dvar = W.moments("plain", 3, P, Xs, grad=True)
                full_v = api.acq_prog_moments(mu, var, prog, q)[0]
                full_a, full_g = api.acq_prog_grad_moments(mu, var, dmu, dvar, prog, q)
                ones = [(api.acq_prog_moments(mu[s], var[s], prog, q)[0],) + api.acq_prog_grad_moments(mu[s], var[s], dmu[s][None], dvar[s][None], prog, q)
                        for s in range(3)]
            else:
                rows = W.rows(kind, 3, P)
                cand = api.Candidates(Xs)
                try:
                    full_v = api.acq_prog(rows, cand, prog, q)[0]
                    vals = [api.acq_prog([rows[s]], cand, prog, q)[0] for s in range(3)]
                finally:
                    cand.close()
                full_a, full_g = api.acq_prog_grad(rows, Xs, prog, q)
                ones = [(vals[s],) + api.acq_prog_grad([rows[s]], Xs, prog, q) for s in range(3)]
            third = 1.0 / 3
            want_v = ((ones[0][0] + ones[1][0]) + ones[2][0]) * third
            want_a = ((ones[0][1] + ones[1][1]) + ones[2][1]) * third
            want_g = ((ones[0][2] + ones[1][2]) + ones[2][2]) * third
            what = (kind, name, M)
            assert same_bits(full_v, want_v) and same_bits(full_a, want_a) and same_bits(full_g, want_g), what
            assert same_bits(full_v, full_a), what


# ------------------------------------------------------------------------------------------ 7. gradient against differences
@pytest.mark.parametrize("kind", ["plain", "kprog", "gradobs", "set"])
def test_gradient_against_central_differences(api, cases, W, kind):
    h = 1e-5
    for name, S in (("pi", 1), ("ucb", 3), ("pi1", 3), ("ucb1", 1)):
        _, P, Q = cases.CLOSURES[name]
        prog, q = cases.programs()[name], np.array([0.2, 1.5, INF, 0.3][:Q])
        Xs = W.Xs[65]                                            # (uniform draws: none sits on a training point)
        rows = W.rows(kind, S, P)
        a, g = api.acq_prog_grad(rows, Xs, prog, q)
        for m in range(D_):
            e = np.zeros((D_, 1))
            e[m] = h
            vals = []
            for sgn in (1.0, -1.0):
                cand = api.Candidates(np.asfortranarray(Xs + sgn * e))
                try:
                    vals.append(api.acq_prog(rows, cand, prog, q)[0])
                finally:
                    cand.close()
            fd = (vals[0] - vals[1]) / (2 * h)
            bar = 1e-6 * np.maximum(1.0, np.abs(g[m]))
            assert np.all(np.abs(fd - g[m]) <= bar), (kind, name, S, m, float(np.max(np.abs(fd - g[m]) / bar)))


# ------------------------------------------------------------------------------------------ 8. plugin level
BETA = 2.0


def _gp_model(B, P, kernel=None):
    kw = {} if kernel is None else {"kernel": kernel}
    return B.HipGaussianProcess(lengthscale_priors=[None] * P, amplitude_priors=[None] * P, noise_std_priors=[None] * P, **kw)


def _params(B, P, S):
    ps = [B.HipGPParams(np.full((2, P), 0.4 + 0.15 * s), [1.0 + 0.1 * s] * P, [0.05] * P) for s in range(3)]
    return ps[0] if S == 1 else ps


def _data(P):
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, (2, N_))
    return X, np.stack([np.sin(3 * X[0]) + X[1], 0.5 * X[0] - X[1] ** 2])[:P]


def _problem(B, acq, model, P, S, f=None):
    X, Y = _data(P)
    return B.BossProblem(f=f, domain=B.Domain(bounds=([0., 0.], [1., 1.])), y_max=[INF, 0.6][:P], acquisition=acq, model=model,
                         data=B.ExperimentData(X, Y), params=_params(B, P, S))


def _grid():
    g1, g2 = np.meshgrid(np.linspace(-0.02, 1.02, 16), np.linspace(0.0, 1.0, 8))
    return np.asfortranarray(np.stack([g1.ravel(), g2.ravel()]))         # 128 points, some outside the bounds


def cases_fold(dm, dv, var, dmu, dvar):
    import acq_program_cases
    return acq_program_cases.fold(dm, dv, var, dmu, dvar)


def ucb_reference(posts, Xs, c, beta, mask):
    """The numpy closure on mean_and_var, samples added in ascending order and scaled once; the bar of test 4 per sample, a BI mean
    adding (S + 1)·u·mean|a_s| as in tests/acq_tails_cases.py."""
    c = np.asarray(c, float)
    vals, bars = [], []
    for p in posts:
        mu, var = p.mean_and_var(Xs)
        vals.append(c @ mu + beta * np.sqrt((c * c) @ var))
        bars.append(8 * U * (np.abs(c @ mu) + beta * np.sqrt((c * c) @ var)))
    S = len(posts)
    acc = vals[0]
    for v in vals[1:]:
        acc = acc + v
    want = acc * (1.0 / S) if S > 1 else acc
    bar = np.mean(bars, axis=0) + ((S + 1) * U * np.mean(np.abs(vals), axis=0) if S > 1 else 0.0)
    return np.where(mask, want, -INF), bar


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("model_kind", ["builtin", "device_kernel"])
def test_maximisers_with_an_upper_confidence_bound(B, model_kind, S):
    from boss_jl_amd.maximizer import posteriors_of
    from boss_jl_amd.problem import in_bounds
    P, c = 2, [1.0, -0.5]
    kernel = None if model_kind == "builtin" else B.DeviceKernel(lambda u, v: np.exp(-0.5 * ((u[0] - v[0]) ** 2 + (u[1] - v[1]) ** 2)), 2, grad=True)
    acq = B.UpperConfidenceBound(B.LinFitness(c), BETA)
    prob = _problem(B, acq, _gp_model(B, P, kernel), P, S)
    pts = _grid()
    mask = in_bounds(pts, prob.domain.bounds)
    posts = posteriors_of(prob)
    try:
        want, bar = ucb_reference(posts, pts, c, BETA, mask)
    finally:
        for p in posts:
            p.close()
    for shard in ("candidates", "outputs", "samples"):
        am = B.HipBatchAM(points=pts, shard=shard)
        _, got = am.maximize_acquisition(prob, return_all=True)
        x, v = am.maximize_acquisition(prob)
        assert np.all(np.isneginf(got[~mask])) and np.all(np.abs(got[mask] - want[mask]) <= bar[mask]), (shard, float(np.max(np.abs(got[mask] - want[mask]) / bar[mask])))
        j = int(np.argmax(got))
        assert np.array_equal(x, pts[:, j]) and v == got[j] and mask[j]
    # the ascent: never below its best start
    prior = lambda r: r.uniform(0.0, 1.0, 2)                      # noqa: E731
    gam = B.HipGradientAM(x_prior=prior, multistart=16, iters=3, seed=3)
    x, v = gam.maximize_acquisition(prob)
    rng = np.random.default_rng(3)
    X0 = np.asfortranarray(np.stack([prior(rng) for _ in range(16)], axis=1))
    posts = posteriors_of(prob)
    try:
        f0, g0 = gam._value_and_grad(prob, posts, X0)
        w0, b0 = ucb_reference(posts, X0, c, BETA, np.ones(16, bool))
    finally:
        for p in posts:
            p.close()
    assert np.all(np.abs(f0 - w0) <= b0) and np.all(np.isfinite(g0)) and np.abs(g0).max() > 0
    assert v >= f0.max() and np.all(x >= 0.0) and np.all(x <= 1.0)
    if model_kind == "builtin":
        xs, _ = B.HipSequentialBatchAM(B.HipBatchAM(points=pts), 2).maximize_acquisition(prob)
        assert xs.shape == (2, 2) and np.array_equal(xs[:, 0], pts[:, int(np.argmax(want))]) and not np.array_equal(xs[:, 0], xs[:, 1])
    else:
        with pytest.raises(NotImplementedError):                 # (as for every acquisition: appends are built-in-kernel only)
            B.HipSequentialBatchAM(B.HipBatchAM(points=pts), 2).maximize_acquisition(prob)


class _FixedFitter:
    def __init__(self, params):
        self.params = params

    def estimate_parameters(self, problem, options=None):
        return self


def _sqexp2(u, v):
    return np.exp(-0.5 * ((u[0] - v[0]) ** 2 + (u[1] - v[1]) ** 2))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("model_kind", ["builtin", "device_kernel"])
def test_bo_runs_two_iterations(B, model_kind, S):
    """bo() with HipBatchAM (UCB) and with HipGradientAM (PI), over a built-in kernel and a DeviceKernel(grad=True).  The nonstationary
    model: test_nonstationary_model_takes_the_moments_path."""
    from boss_jl_amd.bo import bo
    P = 2
    model = lambda: _gp_model(B, P, None if model_kind == "builtin" else B.DeviceKernel(_sqexp2, 2, grad=True))     # noqa: E731
    f = lambda x: [np.sin(3 * x[0]) + x[1], 0.5 * x[0] - x[1] ** 2]     # noqa: E731
    prob = _problem(B, B.UpperConfidenceBound(B.LinFitness([1.0, -0.5]), BETA), model(), P, S, f=f)
    bo(prob, _FixedFitter(_params(B, P, S)), B.HipBatchAM(points=_grid()), 2)
    assert prob.data.X.shape == (2, N_ + 2) and np.all(prob.data.X[:, N_:] >= 0) and np.all(prob.data.X[:, N_:] <= 1)
    grid = _grid()                                               # (noisy observations: UCB may pick a point twice)
    assert all(np.any(np.all(grid == prob.data.X[:, [k]], axis=0)) for k in (N_, N_ + 1)) and np.all(np.isfinite(prob.data.Y))
    prob = _problem(B, B.ProbabilityOfImprovement(B.LinFitness([1.0, -0.5]), 0.01), model(), P, S, f=f)
    bo(prob, _FixedFitter(_params(B, P, S)), B.HipGradientAM(x_prior=lambda r: r.uniform(0.0, 1.0, 2), multistart=8, iters=3, seed=1), 2)
    assert prob.data.X.shape == (2, N_ + 2)


@pytest.mark.parametrize("S", [1, 3])
def test_nonstationary_model_takes_the_moments_path(B, S):
    """A HipNonstationaryGP on a MAP fit and on 3 samples.  Its posteriors reach a maximiser only as `posts=`: the model's
    model_posterior(data) / model_posterior_slice(data, i) are not the (params, data[, reserve]) calls posteriors_of and
    output_moments make, for any acquisition.  So acquisition_values, HipBatchAM(shard="candidates") and HipGradientAM run here, and
    what builds its own posteriors — shard="outputs" / "samples", HipSequentialBatchAM, bo() — is asserted to stop with that
    TypeError, before any device work, as it does for ExpectedImprovement."""
    from boss_jl_amd.bo import bo
    from boss_jl_amd.maximizer import acquisition_values
    from boss_jl_amd.model import HipGaussianProcessPosterior
    rng = np.random.default_rng(4)
    d, N, M = 2, 64, 65
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3 * X[0]) + X[1], 0.5 * X[0] - X[1] ** 2])
    data = B.ExperimentData(X, Y)
    models = [B.HipNonstationaryGP([lambda x, k=k: 0.4 + 0.1 * k + 0.2 * np.asarray(x) ** 2] * 2, [lambda x: 1.0 + 0.3 * np.sin(np.sum(x))] * 2,
                                   [lambda x: 0.05] * 2) for k in range(S)]
    posts = [HipGaussianProcessPosterior(m.model_posterior(data)) for m in models]
    c = [1.0, -0.5]
    mk = lambda acq: B.BossProblem(f=None, domain=B.Domain(bounds=([0., 0.], [1., 1.])), y_max=[INF, 0.6], model=models[0], data=data,     # noqa: E731
                                   acquisition=acq)
    prob = mk(B.UpperConfidenceBound(B.LinFitness(c), BETA))
    try:
        Xs = np.asfortranarray(rng.uniform(-0.02, 1.02, (d, M)))
        mask = B.problem.in_bounds(Xs, prob.domain.bounds)
        want, bar = ucb_reference(posts, Xs, c, BETA, mask)
        got, am, mx = acquisition_values(prob, posts, Xs)
        assert np.all(np.isneginf(got[~mask])) and np.all(np.abs(got[mask] - want[mask]) <= bar[mask])
        assert am == int(np.argmax(got)) and mx == got[am]
        x, v = B.HipBatchAM(points=Xs).maximize_acquisition(prob, posts=posts)
        assert np.array_equal(x, Xs[:, am]) and v == mx
        gam = B.HipGradientAM(x_prior=lambda r: r.uniform(0.0, 1.0, 2), multistart=8, iters=3, seed=1)
        Xin = np.asfortranarray(Xs[:, mask][:, :8])
        f0, g0 = gam._value_and_grad(prob, posts, Xin)
        assert np.all(np.abs(f0 - want[mask][:8]) <= bar[mask][:8]) and np.all(np.isfinite(g0)) and np.abs(g0).max() > 0
        # the gradient is the reverse sweep folded with the slices' own moment gradients, samples in ascending order
        prog, gs = prob.acquisition.program, []
        for p in posts:
            mvg = [s.mean_and_var_grad(Xin) for s in p.slices]
            mu, var, dmu, dvar = (np.stack([r[k] for r in mvg]) for k in range(4))
            _, dm, dv = prog.eval_host(mu, var, want_grad=True)
            gs.append(cases_fold(dm, dv, var, dmu, dvar))
        gw = gs[0] if S == 1 else ((gs[0] + gs[1]) + gs[2]) * (1.0 / 3)
        # (the same adjoints folded in the same order; the device may fuse a product into the running sum: a few u of the addends)
        assert np.all(np.abs(g0 - gw) <= 1e-13 * np.maximum(1.0, np.abs(gw)))
        x, v = gam.maximize_acquisition(prob, posts=posts)
        assert np.all(x >= 0.0) and np.all(x <= 1.0) and np.isfinite(v)
        # what builds its own posteriors stops at the model's interface, for this acquisition as for ExpectedImprovement
        for acq in (prob.acquisition, B.ExpectedImprovement(B.LinFitness(c))):
            pr = mk(acq)
            for shard in ("outputs", "samples"):
                with pytest.raises(TypeError, match="model_posterior"):
                    B.HipBatchAM(points=Xs, shard=shard).maximize_acquisition(pr, posts=posts)
            with pytest.raises(TypeError, match="model_posterior"):
                B.HipSequentialBatchAM(B.HipBatchAM(points=Xs), 2).maximize_acquisition(pr)
            with pytest.raises(TypeError, match="model_posterior"):
                bo(pr, _FixedFitter(None), B.HipBatchAM(points=Xs, fused=False), 1)
    finally:
        for p in posts:
            p.close()


def test_samples_shard_takes_a_map_fit_for_expected_improvement_too(B):
    """shard="samples" with one parameter set (a MAP fit is one sample): the result of shard="candidates", for the built-in EI."""
    P, pts = 2, _grid()
    prob = _problem(B, B.ExpectedImprovement(B.LinFitness([1.0, -0.5])), _gp_model(B, P), P, 1)
    _, want = B.HipBatchAM(points=pts, fused=False).maximize_acquisition(prob, return_all=True)
    _, got = B.HipBatchAM(points=pts, shard="samples").maximize_acquisition(prob, return_all=True)
    xw, vw = B.HipBatchAM(points=pts, fused=False).maximize_acquisition(prob)
    xg, vg = B.HipBatchAM(points=pts, shard="samples").maximize_acquisition(prob)
    assert same_bits(got, want) and want.max() > 0 and np.array_equal(xg, xw) and vg == vw


@pytest.mark.parametrize("S", [1, 3])
def test_ei_as_a_device_acquisition_picks_the_point_expected_improvement_picks(B, cases, S):
    P, c = 2, [1.0, -0.5]
    pts = _grid()
    pe = _problem(B, B.ExpectedImprovement(B.LinFitness(c)), _gp_model(B, P), P, S)
    pd = _problem(B, cases.ei_fp_acquisition(c), _gp_model(B, P), P, S)
    am = B.HipBatchAM(points=pts, fused=False)
    xe, ve = am.maximize_acquisition(pe)
    xd, vd = am.maximize_acquisition(pd)
    _, ae = am.maximize_acquisition(pe, return_all=True)
    _, ad = am.maximize_acquisition(pd, return_all=True)
    print(f"S={S}: max|EI program - EI| = {np.abs(ad - ae).max():.3e}, max EI {ve:.3e}")
    assert np.array_equal(xd, xe) and int(np.argmax(ad)) == int(np.argmax(ae))
