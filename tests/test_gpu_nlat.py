"""Resident latent models of a NonstationaryGP (boss_nlat_*) and the _lat prediction calls that read them on the device
(pytest -m gpu).

1 the raw kernel (target none, identity) against the oracle's gp_fit + gp_mean_and_var_grad (mu, dmu) per latent, by the project's
  parity rule (tests/test_gpu_parity.py:2066-2083): tol = max(1e-9, cond(K) N 2^-53 8), |Δm| <= tol (1 + max|m|),
  |Δ∇m| <= 10 tol (1 + max|∇m|);
2 every target × activation against the numpy closed form and chain rule (B.latent_transform, pinned against scipy in
  tests/test_nlat_host.py) applied to the oracle's (m, ∇m): |Δv| <= |v'(m)| tol (1 + max|m|) + 8 ulp |v|, and with the factor 10
  (and max|∇m|) on the gradients;
3 every _lat call bit for bit against its array twin fed boss_nlat_eval's arrays;
4 the public interface (HipNonstationaryGP(resident_latents=True)) against the oracle's nonstationary posterior fed the closed-form
  latent values and Jacobians, tolerances as tests/test_gpu_ngp_grad_set.py states them;
5 errors.

Shapes: N in {1, 70, 257} and 131 = 2 NLAT_CHUNK + 3 (NLAT_CHUNK = 64 rows are staged per step, latent_kernels.hpp), M in {1, 33, 224}
(one lane of one tile, a second partial tile, seven tiles), d in {1, 3, 16}.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLAT_CHUNK = 64
ULP = 2.0 ** -52
MODES = ("both", "best_only", "cons_only", "none")
TARGETS = {"none": (0.0, 0.0), "normal": (1.0, 0.3), "lognormal": (-0.7, 0.5), "uniform": (0.2, 2.0)}
ACTS = {"identity": 0.0, "softplus": 0.1, "exp": 0.0}
RAW = ("none", (0.0, 0.0), "identity", 0.0)
SAFE = ("lognormal", (-0.7, 0.5), "softplus", 0.1)
# latent models under which the Gibbs systems of the consumer tests stay well conditioned (cond(K) ≈ 2e3-4e3 with the oracle):
# λ ≈ 0.3-0.5 on the unit cube, σ ≈ 0.13
LAM = ("lognormal", (-1.5, 0.4), "identity", 0.0)
NOI = ("normal", (0.1, 0.02), "identity", 0.0)


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


class Latent:
    """One latent GP: N points in [0, 1]^d (×3 where discrete), positive observations (so that the raw posterior mean is a valid
    lengthscale inside the data's range), fitted on the device and by the oracle."""

    def __init__(self, api, O, d, N, kernel, rng, scale=1.0, spec=RAW):
        self.X = rng.uniform(0, 1, (d, N)) * scale
        self.y = 1.5 + 0.3 * np.sin(3 * self.X.sum(0)) + 0.1 * rng.standard_normal(N)
        self.lam = rng.uniform(0.4, 0.9, d) * (np.ravel(scale) if np.ndim(scale) else scale)
        self.amp, self.noise, self.kernel, self.spec, self.N = 1.3, 0.1, kernel, spec, N
        self.gp = api.GP(self.X, self.y, kernel)
        self.gp.update(self.lam, self.amp, self.noise)
        self.post = O.gp_fit(self.X, self.y, kernel, self.lam, self.amp, self.noise)
        self.tol = max(1e-9, np.linalg.cond(self.post.L @ self.post.L.T) * N * 2.0 ** -53 * 8)
        self.arg = (self.gp, spec)

    def oracle(self, O, Xs):
        mu, _, dmu, _ = O.gp_mean_and_var_grad(self.post, Xs)
        return mu, dmu

    def close(self):
        self.gp.close()


def rounded(Z, disc):
    return Z if disc is None else np.where(np.asarray(disc, bool)[:, None], np.rint(Z), Z)


def check_latent(B, O, lat, Xs_seen, v, J, what, zero_cols=None):
    """value row v[M] and Jacobian J[d, M] of one latent against the closed form on the oracle's (m, ∇m)"""
    if not isinstance(lat, Latent):
        assert np.all(v == lat) and (J is None or np.all(J == 0.0)), what
        return
    m, dm = lat.oracle(O, Xs_seen)
    v_o, dv = B.latent_transform(lat.spec, m)
    bound = np.abs(dv) * lat.tol * (1 + np.abs(m).max()) + 8 * ULP * np.abs(v_o)
    err = np.abs(v - v_o)
    print(f"{what}: value {err.max():.2e} (<= {bound[np.argmax(err)]:.2e})", end="")
    assert np.all(err <= bound), (what, err.max())
    if J is not None:
        J_o = dv[None, :] * dm
        if zero_cols is not None:
            J_o[zero_cols] = 0.0
            assert np.all(J[zero_cols] == 0.0), what
        boundJ = 10 * np.abs(dv)[None, :] * lat.tol * (1 + np.abs(dm).max()) + 8 * ULP * np.abs(J_o)
        errJ = np.abs(J - J_o)
        print(f"  Jacobian {errJ.max():.2e} (<= {boundJ.flat[np.argmax(errJ)]:.2e})", end="")
        assert np.all(errJ <= boundJ), (what, errJ.max())
    print(flush=True)


def check_object(B, O, lats, L, Xs, disc, what, noise=True):
    """every latent of one NgpLatents at Xs; lats = d + 2 entries (Latent, float or None)"""
    d = Xs.shape[0]
    lam, amp, noi, dl, da = L.eval(Xs, jac=True, noise=noise and lats[d + 1] is not None)
    Xr = rounded(Xs, disc)
    zc = None if disc is None else np.asarray(disc, bool)
    for q in range(d):
        check_latent(B, O, lats[q], Xr, lam[q], dl[q], f"{what} lam[{q}]", zc)
    check_latent(B, O, lats[d], Xr, amp, da, f"{what} amp", zc)
    if noi is not None:
        check_latent(B, O, lats[d + 1], Xs, noi, None, f"{what} noise")       # σ sees the point as given
    return lam, amp, noi, dl, da


def build(api, lats, disc=None):
    d = len(lats) - 2
    arg = [x.arg if isinstance(x, Latent) else x for x in lats]
    return api.NgpLatents(arg[:d], arg[d], arg[d + 1], disc)


# ------------------------------------------------------------------------------------------ 1: the raw kernel
@pytest.mark.parametrize("kernel,d,Ns,M", [("matern32", 3, (70, None, 257, 131, 70), 33), ("matern52", 3, (257, 131, None, 70, None), 224),
                                           ("sqexp", 3, (131, 70, 1, None, 257), 33), ("matern52", 1, (1, None, 1), 1),
                                           ("matern32", 16, (1, 70, 131) * 5 + (None, 257, None), 224)])
def test_raw_kernel_against_the_oracle(api, O, B, kernel, d, Ns, M):
    """Target none, identity: λ rows / α / σ and their Jacobians are the latent posteriors' (mu, dmu).  Ns: points of latent q (None:
    a constant).  The first candidate lies exactly on a training point of the first GP latent (zero gradient contribution, no NaN)."""
    rng = np.random.default_rng(100 * d + M)
    lats = [0.7 + 0.1 * q if N is None else Latent(api, O, d, N, kernel, rng) for q, N in enumerate(Ns)]
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
    first = next(x for x in lats if isinstance(x, Latent))
    Xs[:, 0] = first.X[:, 0]
    L = build(api, lats)
    try:
        out = check_object(B, O, lats, L, Xs, None, f"{kernel} d={d} M={M}")
        assert all(np.all(np.isfinite(a)) for a in out if a is not None)
        again = L.eval(Xs, jac=True, noise=lats[d + 1] is not None)
        assert all(np.array_equal(a, b) for a, b in zip(out, again) if a is not None)
    finally:
        L.close()
        for x in lats:
            if isinstance(x, Latent):
                x.close()


def test_discrete_dimension_rounds_for_lam_and_amp_only(api, O, B):
    """d = 3 with the middle dimension discrete, points and candidates ×3 there: λ, α see the rounded candidate and have a zero
    Jacobian column, σ sees the candidate as given."""
    rng = np.random.default_rng(5)
    disc = [False, True, False]
    scale = np.array([1.0, 3.0, 1.0])[:, None]
    lats = [Latent(api, O, 3, N, "matern52", rng, scale) for N in (70, 131, 70, 257, 70)]
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (3, 33)) * scale)
    assert np.abs(np.rint(Xs[1]) - Xs[1]).min() > 1e-3
    L = build(api, lats, disc)
    try:
        lam, amp, noi, dl, da = check_object(B, O, lats, L, Xs, disc, "discrete")
        assert np.all(dl[:, 1, :] == 0.0) and np.all(da[1] == 0.0) and np.abs(dl[:, 0, :]).min() > 0
    finally:
        L.close()
        for x in lats:
            x.close()


# ------------------------------------------------------------------------------------------ 2: transforms
@pytest.fixture(scope="module")
def two_gps(api, O):
    rng = np.random.default_rng(11)
    a, b = Latent(api, O, 2, 131, "matern52", rng), Latent(api, O, 2, 70, "matern32", rng)
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("act", list(ACTS))
def test_transforms(api, O, B, two_gps, target, act):
    a, b = two_gps
    spec = (target, TARGETS[target], act, ACTS[act])
    rng = np.random.default_rng(3)
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (2, 33)))
    lats = []
    for g in (a, b, a, b):
        t = Latent.__new__(Latent)
        t.__dict__.update(g.__dict__, spec=spec, arg=(g.gp, spec))
        lats.append(t)
    L = build(api, lats)
    try:
        check_object(B, O, lats, L, Xs, None, f"{target}/{act}")
    finally:
        L.close()


def test_softplus_is_overflow_safe(api, O, B):
    """z = 800 m through softplus: exp(z) overflows, the closed form does not (value ≈ z, derivative = 800 σ(z) = 800)."""
    rng = np.random.default_rng(2)
    g = Latent(api, O, 1, 70, "sqexp", rng, spec=("normal", (0.0, 800.0), "softplus", 0.0))
    L = build(api, [g, 1.0, None])
    try:
        Xs = np.asfortranarray(rng.uniform(0.1, 0.9, (1, 33)))
        lam, _, _, dl, _ = L.eval(Xs)
        m, dm = g.oracle(O, Xs)
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(dl)) and (800 * m).min() > 710
        assert np.allclose(lam[0], 800 * m, rtol=1e-9) and np.allclose(dl[0], 800 * dm, rtol=1e-6, atol=1e-6)
    finally:
        L.close()
        g.close()


# ------------------------------------------------------------------------------------------ 3: consumers, bit for bit
class Members:
    """S × P nonstationary posteriors (per output the members of one ngp_fit_batch on N points; members s >= S/2 on the first N_alt
    points when given), each with its own resident latent models: λ_0, λ_2 GP posteriors through LAM, λ_1 a constant, α through
    SAFE, σ through NOI."""

    def __init__(self, api, O, N=70, M=33, S=4, P=2, d=3, disc=None, N_alt=None, seed=0):
        rng = np.random.default_rng(900 + seed)
        self.S, self.P, self.d, self.M, self.n, self.disc = S, P, d, M, S * P, disc
        scale = np.where(np.asarray(disc, bool), 3.0, 1.0)[:, None] if disc is not None else 1.0
        self.X = rng.uniform(0, 1, (d, N)) * scale
        self.Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)) * scale)
        self.Y = np.stack([np.sin(3 * self.X).sum(0), self.X[0] - self.X[1] + 0.2 * np.cos(4 * self.X[2])])[:P]
        self.latgps, self.lats = [], [[None] * P for _ in range(S)]
        self.gps = [[None] * P for _ in range(S)]
        for s in range(S):
            for p in range(P):
                ls = [Latent(api, O, d, n_, "matern52", rng, scale, sp) for n_, sp in ((70, LAM), (40, LAM), (131, SAFE))]
                self.latgps += ls
                noise = Latent(api, O, d, 40, "matern32", rng, scale, NOI)
                self.latgps.append(noise)
                self.lats[s][p] = build(api, [ls[0], 0.6 + 0.05 * s, ls[1], ls[2], noise], disc)
        for p in range(P):
            groups = [(list(range(S)), N)] if N_alt is None else [(list(range(S // 2)), N), (list(range(S // 2, S)), N_alt)]
            for members, Nn in groups:
                lamX = np.empty((d, Nn, len(members)), order="F")
                ampX, noiX = np.empty((Nn, len(members)), order="F"), np.empty((Nn, len(members)), order="F")
                for q, s in enumerate(members):
                    lamX[:, :, q], ampX[:, q], noiX[:, q], _, _ = self.lats[s][p].eval(self.X[:, :Nn], jac=False, noise=True)
                gp, _, st = api.ngp_fit_batch(self.X[:, :Nn], self.Y[p, :Nn], lamX, ampX, noiX, None, disc)
                assert not st.any()
                for q, s in enumerate(members):
                    self.gps[s][p] = gp[q]
        self.ms = rng.uniform(-0.2, 0.2, (self.n, M))
        self.mg = rng.uniform(-0.2, 0.2, (self.n, d, M))
        self.mask = np.ones(M, bool)
        self.mask[::7] = False
        self.coefs = [1.0, 0.2][:P]
        self.y_max = [np.inf, 0.3][:P]
        self.best = 0.4

    def flat(self):
        return [self.gps[s][p] for s in range(self.S) for p in range(self.P)]

    def flat_lats(self):
        return [self.lats[s][p] for s in range(self.S) for p in range(self.P)]

    def arrays(self):
        d, M, n = self.d, self.M, self.n
        lam, amp = np.empty((d, M, n), order="F"), np.empty((M, n), order="F")
        dl, da = np.empty((d, d, M, n), order="F"), np.empty((d, M, n), order="F")
        for i, L in enumerate(self.flat_lats()):
            lam[:, :, i], amp[:, i], _, dl[:, :, :, i], da[:, :, i] = L.eval(self.Xs)
        return lam, amp, dl, da

    def close(self):
        for row in self.gps:
            for g in row:
                g.close()
        for row in self.lats:
            for L in row:
                L.close()
        for g in self.latgps:
            g.close()


def same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, k, np.abs(np.asarray(x) - np.asarray(y)).max())


def check_set_calls(api, c, what, expect_set=None):
    lam, amp, dl, da = c.arrays()
    before = api._set_grad_launches()
    same(api.ngp_predict_set_lat(c.flat(), c.Xs, c.flat_lats(), c.ms), api.ngp_predict_set(c.flat(), c.Xs, lam, amp, c.ms), what + " predict_set")
    r1 = api.ngp_predict_grad_set_lat(c.flat(), c.Xs, c.flat_lats(), c.ms, c.mg)
    same(r1, api.ngp_predict_grad_set(c.flat(), c.Xs, lam, amp, dl, da, c.ms, c.mg), what + " predict_grad_set")
    same(r1, api.ngp_predict_grad_set_lat(c.flat(), c.Xs, c.flat_lats(), c.ms, c.mg), what + " twice")
    assert np.abs(r1[2]).max() > 0 and np.all(np.isfinite(r1[3]))
    for y_max, best in ((c.y_max, c.best), (None, c.best)):
        a1 = api.ngp_acq_ei_grad_set_lat(c.gps, c.Xs, c.lats, c.coefs, y_max, best, c.mask, c.ms, c.mg)
        same(a1, api.ngp_acq_ei_grad_set(c.gps, c.Xs, lam, amp, dl, da, c.coefs, y_max, best, c.mask, c.ms, c.mg), what + " acq")
        same(a1, api.ngp_acq_ei_grad_set_lat(c.gps, c.Xs, c.lats, c.coefs, y_max, best, c.mask, c.ms, c.mg), what + " acq twice")
        assert np.abs(a1[1]).max() > 0
    if expect_set is True:
        assert api._set_grad_launches() > before
    elif expect_set is False:
        assert api._set_grad_launches() == before


@pytest.fixture(scope="module")
def members(api, O):
    c = Members(api, O)
    yield c
    c.close()


def test_single_handle_calls_equal_their_array_twins(api, members):
    c = members
    for i, (g, L) in enumerate(zip(c.flat(), c.flat_lats())):
        lam, amp, _, dl, da = L.eval(c.Xs)
        same(g.predict_lat(c.Xs, L, c.ms[i]), g.predict(c.Xs, lam, amp, c.ms[i]), f"predict {i}")
        r = g.predict_grad_lat(c.Xs, L, c.ms[i], c.mg[i])
        same(r, g.predict_grad(c.Xs, lam, amp, dl, da, c.ms[i], c.mg[i]), f"predict_grad {i}")
        same(r, g.predict_grad_lat(c.Xs, L, c.ms[i], c.mg[i]), f"predict_grad twice {i}")
    # one candidate (the one-lane tile)
    g, L = c.gps[0][0], c.lats[0][0]
    lam, amp, _, dl, da = L.eval(c.Xs[:, :1])
    same(g.predict_grad_lat(c.Xs[:, :1], L), g.predict_grad(c.Xs[:, :1], lam, amp, dl, da), "one candidate")


def test_set_calls_equal_their_array_twins(api, members):
    check_set_calls(api, members, "set", expect_set=True)


def test_set_calls_with_a_discrete_dimension(api, O):
    c = Members(api, O, S=2, disc=[False, True, False], seed=1)
    try:
        check_set_calls(api, c, "discrete", expect_set=True)
        r = api.ngp_predict_grad_set_lat(c.flat(), c.Xs, c.flat_lats())
        assert np.all(r[2][:, 1, :] == 0.0) and np.all(r[3][:, 1, :] == 0.0)
    finally:
        c.close()


def test_members_of_two_shapes_go_member_by_member(api, O):
    c = Members(api, O, N_alt=60, seed=2)
    try:
        check_set_calls(api, c, "two shapes", expect_set=False)
    finally:
        c.close()


CHILD = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from boss_jl_amd import api
from oracle import gp_oracle as O
import test_gpu_nlat as T
c = T.Members(api, O, S=2)
T.check_set_calls(api, c, "BOSS_NO_SET_PREDICT=1", expect_set=False)
assert api._set_grad_launches() == 0
c.close()
print("CHILD_OK")
'''


def test_no_set_predict_switch_goes_member_by_member(api):
    env = dict(os.environ, BOSS_NO_SET_PREDICT="1")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------ 4: end to end against the oracle
class EndToEnd:
    """S models × P outputs of HipNonstationaryGP(resident_latents=True) whose latents are HipParametrizedGP posteriors (LogNormal
    target for λ_0, λ_2, softplus on a Normal target for α, λ_1 and σ constants) on N points; the oracle's nonstationary posterior
    is fed the closed-form latent values and Jacobians computed from the oracle's own latent posteriors."""

    def __init__(self, api, O, B, N=70, M=33, S=2, P=2, d=3, Nl=40):
        from scipy import stats
        from boss_jl_amd.problem import ExperimentData
        rng = np.random.default_rng(77)
        self.S, self.P, self.d, self.M, self.n = S, P, d, M, S * P
        X = rng.uniform(0, 1, (d, N))
        self.Xs = Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
        self.Y = Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1] + 0.2 * np.cos(4 * X[2])])[:P]
        data, ldata = ExperimentData(X, Y), ExperimentData(rng.uniform(0, 1, (d, Nl)), np.zeros((1, Nl)))
        pg_lam = B.HipParametrizedGP(np.full(d, 0.6), "matern52", stats.lognorm(0.2, scale=np.exp(-1.0)), B.identity_act, 0.1)
        pg_amp = B.HipParametrizedGP(np.full(d, 0.7), "matern32", stats.norm(0.8, 0.4), B.softplus.with_lower_bound(0.05), 0.1)
        self.models, self.closers = [], []
        lamX, ampX = np.empty((S, P, d, N)), np.empty((S, P, N))
        self.lamS, self.ampS = np.empty((d, M, self.n), order="F"), np.empty((M, self.n), order="F")
        self.Dl, self.Da = np.zeros((d, d, M, self.n), order="F"), np.zeros((d, M, self.n), order="F")

        def latent(pg, i, Z, grad):
            """(closure, values at the training points, values at Xs, Jacobian at Xs) of one sampled ParametrizedGP"""
            prm = pg.params_sampler(ldata)(rng)
            post = pg.model_posterior(prm)
            self.closers.append(post)
            op = O.gp_fit(prm.X, prm.L @ prm.yeps, pg.kernel, prm.lengthscale, 1.0, pg.noise_std)
            spec = pg.device_spec()
            vX = B.latent_transform(spec, O.gp_mean_and_var(op, X, clip=False)[0])[0]
            m, _, dm, _ = O.gp_mean_and_var_grad(op, Xs)
            v, dv = B.latent_transform(spec, m)
            return post, vX, v, dv[None, :] * dm

        for s in range(S):
            fl, fa, fn = [], [], []
            for p in range(P):
                i = p + P * s
                l0, l2, a = latent(pg_lam, i, X, True), latent(pg_lam, i, X, True), latent(pg_amp, i, X, True)
                c1 = 0.5 + 0.1 * s
                fl.append(B.stack_latents([l0[0], B.constant_latent(c1), l2[0]]))
                fa.append(a[0])
                fn.append(B.constant_latent(0.3))
                lamX[s, p] = np.stack([l0[1], np.full(N, c1), l2[1]])
                ampX[s, p] = a[1]
                self.lamS[:, :, i] = np.stack([l0[2], np.full(M, c1), l2[2]])
                self.ampS[:, i] = a[2]
                self.Dl[0, :, :, i], self.Dl[2, :, :, i], self.Da[:, :, i] = l0[3], l2[3], a[3]
            self.models.append(B.HipNonstationaryGP(fl, fa, fn, resident_latents=True))
        self.posts = B.nonstationary_model_posterior_batch(self.models, data)
        self.tol = np.empty((S, P))
        self.full = [None] * self.n
        for s in range(S):
            for p in range(P):
                i = p + P * s
                post = O.nonstationary_fit(X, Y[p], lamX[s, p], ampX[s, p], np.full(N, 0.3))
                self.tol[s, p] = max(1e-9, np.linalg.cond(post.L @ post.L.T) * N * 2.0 ** -53 * 8)
                self.full[i] = O.nonstationary_mean_and_var_grad(post, Xs, self.lamS[:, :, i], self.ampS[:, i], self.Dl[:, :, :, i],
                                                                 self.Da[:, :, i])
        self.mask = np.ones(M, bool)
        self.mask[::7] = False
        self.coefs = [1.0, 0.2][:P]

    def args(self, O, mode):
        return _T().Case.args(self, O, mode)

    def oracle_acq(self, O, mode, moments=None):
        return _T().Case.oracle_acq(self, O, mode, moments)

    def close(self):
        for row in self.posts:
            for sl in row:
                sl.close()
        for c in self.closers:
            c.close()


def _T():
    """tests/test_gpu_ngp_grad_set.py: its composition of the oracle's acquisition and its bounds are reused as they stand"""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_ngp_grad_set as T
    return T


def test_end_to_end_against_the_oracle(api, O, B):
    """mean_and_var_grad of every slice by the rule of tests/test_gpu_ngp_grad_set.py (|Δμ| <= tol (1 + max|μ|), |Δσ²| <= tol max α*²,
    |Δ∇| <= 10 tol (1 + max|∇|)), nonstationary_acq_ei_grad_batch in the four modes by its acquisition rule (|Δacq| <= 10 tol,
    |Δ∇acq| <= 100 tol (1 + max|∇acq|), tol summed over a sample's members, mean over s), mean_and_var and mean_and_cov beside them."""
    T = _T()
    e = EndToEnd(api, O, B)
    try:
        assert all(sl.latents is not None for row in e.posts for sl in row)
        for s in range(e.S):
            for p in range(e.P):
                i = p + e.P * s
                tol = e.tol[s, p]
                mu, var, dmu, dvar = e.posts[s][p].mean_and_var_grad(e.Xs)
                mu_o, var_o, dmu_o, dvar_o = e.full[i]
                errs = (np.abs(mu - mu_o).max(), np.abs(var - np.maximum(var_o, 0.0)).max(), np.abs(dmu - dmu_o).max(), np.abs(dvar - dvar_o).max())
                bounds = (tol * (1 + np.abs(mu_o).max()), tol * e.ampS[:, i].max() ** 2, 10 * tol * (1 + np.abs(dmu_o).max()),
                          10 * tol * (1 + np.abs(dvar_o).max()))
                print(f"slice {s},{p}: " + "  ".join(f"{a:.2e} (<= {b:.2e})" for a, b in zip(errs, bounds)), flush=True)
                assert all(a <= b for a, b in zip(errs, bounds)), (s, p, errs, bounds)
                mu2, var2 = e.posts[s][p].mean_and_var(e.Xs)
                assert np.abs(mu2 - mu_o).max() <= bounds[0] and np.abs(var2 - np.maximum(var_o, 0.0)).max() <= bounds[1]
                mu3, cov = e.posts[s][p].mean_and_cov(e.Xs)
                assert np.abs(mu3 - mu_o).max() <= bounds[0] and np.abs(np.diag(cov) - np.maximum(var_o, 0.0)).max() <= bounds[1]
        for mode in MODES:
            y_max, b = e.args(O, mode)
            res = B.nonstationary_acq_ei_grad_batch(e.posts, e.Xs, e.coefs, y_max, b, e.mask)
            T.assert_acq(e, O, res, mode, "resident")
            if mode != "none":
                acq = B.nonstationary_acq_ei_batch(e.posts, e.Xs, e.coefs, y_max, b, e.mask)[0]
                assert np.abs(acq - res[0])[e.mask].max() <= 2 * e.oracle_acq(O, mode)[2]
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5: errors
def test_errors(api, O, members):
    c = members
    rng = np.random.default_rng(8)
    g, L = c.gps[0][0], c.lats[0][0]
    ref = g.predict_grad_lat(c.Xs, L)
    # a latent whose transform goes non-positive at ONE candidate: Normal target with a negative mean on a GP that is ≈ 1.5 near its
    # data and ≈ 0 far from it: λ = -0.5 + m
    lg = Latent(api, O, c.d, 70, "sqexp", rng, spec=("normal", (-0.5, 1.0), "identity", 0.0))
    bad = api.NgpLatents([(lg.gp, lg.spec), 0.6, 0.6], 1.0)
    Xs = c.Xs.copy(order="F")
    Xs[:, 5] = 40.0                                              # far from every training point: m = 0, λ = -0.5
    m = lg.oracle(O, Xs)[0]
    assert m[5] < 0.4 and np.delete(m, 5).min() > 0.6
    with pytest.raises(api.BossError) as e:
        bad.eval(Xs)
    assert e.value.code == api.BOSS_E_INVALID and e.value.bad_index == 5
    for call in (lambda: g.predict_lat(Xs, bad), lambda: g.predict_grad_lat(Xs, bad),
                 lambda: api.ngp_predict_set_lat(c.flat(), Xs, [bad] * c.n),
                 lambda: api.ngp_predict_grad_set_lat(c.flat(), Xs, c.flat_lats()[:-1] + [bad]),
                 lambda: api.ngp_acq_ei_grad_set_lat(c.gps, Xs, [[bad] * c.P] * c.S, c.coefs, None, 0.1)):
        with pytest.raises(api.BossError) as e:
            call()
        assert e.value.code == api.BOSS_E_INVALID
        same(g.predict_grad_lat(c.Xs, L), ref, "after an invalid latent value")
    assert np.all(np.isfinite(bad.eval(c.Xs)[0]))                # the object itself stays usable
    bad.close()
    # mismatched discrete flags / x_dim
    flagged = api.NgpLatents([0.5, 0.5, 0.5], 1.0, None, [False, True, False])
    two = api.NgpLatents([0.5, 0.5], 1.0)
    for other in (flagged, two):
        for call in (lambda: g.predict_lat(c.Xs, other), lambda: g.predict_grad_lat(c.Xs, other),
                     lambda: api.ngp_predict_grad_set_lat(c.flat(), c.Xs, [other] * c.n)):
            with pytest.raises(api.BossError) as e:
                call()
            assert e.value.code == api.BOSS_E_INVALID
    flagged.close()
    two.close()
    # a wrong handle kind and an unfitted latent
    with pytest.raises(api.BossError) as e:
        api.NgpLatents([(g, RAW), 0.5, 0.5], 1.0)
    assert e.value.code == api.BOSS_E_INVALID
    unfitted = api.GP(lg.X, lg.y, "sqexp")
    with pytest.raises(api.BossError) as e:
        api.NgpLatents([(unfitted, RAW), 0.5, 0.5], 1.0)
    assert e.value.code == api.BOSS_E_NOT_FITTED
    unfitted.close()
    # a plain handle where a nonstationary one belongs
    with pytest.raises(api.BossError) as e:
        api.ngp_predict_set_lat([lg.gp], c.Xs, [L])
    assert e.value.code == api.BOSS_E_INVALID
    same(g.predict_grad_lat(c.Xs, L), ref, "after the errors")
    # updating, then freeing the latent handles after create does not change eval
    good = api.NgpLatents([(lg.gp, SAFE), 0.6, (lg.gp, LAM)], (lg.gp, SAFE), (lg.gp, NOI))
    before = good.eval(c.Xs, noise=True)
    lg.gp.update(lg.lam * 2, 0.5, 0.3)
    same(good.eval(c.Xs, noise=True), before, "after an update of the latent handle")
    lg.close()
    same(good.eval(c.Xs, noise=True), before, "after freeing the latent handle")
    good.close()
