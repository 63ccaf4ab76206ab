"""Shared by tests/test_neg_var_host.py and tests/test_gpu_neg_var.py: inputs that put a posterior variance below zero on demand, what
include/bosship.h promises for them (_clip_var, gaussian_process.jl:186-194: a variance in [-1e-8, 0) becomes 0, below that the call
fails with BOSS_E_NEG_VAR and *bad_index = the first such candidate, "mu/var are still written (var unclipped at the offending
entries)"; in the acquisition calls such a candidate is -Inf with a zero gradient), and the C entry points called without the api.py
wrappers, which drop mu and var when they raise.

Construction A (exact; program-kernel handles).  `flagged` is a squared exponential on all but the last coordinate minus the
product of the last ("flag") coordinates.  Every training point has flag 0, so K and K* are those of a squared exponential, while
k(x*, x*) = α̃²(1 − t²), t the candidate's scaled flag, α̃ = α + 1e-8.  Candidate kinds:
  "H"      flag 0, spatial coordinates in [0, 1]: healthy;
  "P"      flag 1.5(λ_f + 1e-8): σ² between −2.25α̃² and −1.25α̃², offending by a wide margin;
  a float  a far candidate, spatial coordinates 40: K* = 0 exactly (exp underflows, the flag product has a zero factor), so
           μ = 0 and σ² = α̃²(1 − t²) + 1e-18 with no substitution error; the flag is chosen so that σ² = the float.
Far targets −0.99e-8 and −5e-9 must come back as exactly 0.0; −1.01e-8 and −2e-8 offend and come back unclipped, +5e-9 as it is,
each within FAR_BAR·α̃² of the target: four roundings (scaling, square, subtraction, amplitude) with a factor two, far below the
1e-10 between a target and the threshold.

Construction B (rounding-driven; built-in kernels, d = 1).  X = 10·arange(N) + U(0, 4), y = sin X, λ = 3, α = 1e5, σ = 1e-4;
candidates: 37 midpoints X[:37] + 5, then the training points themselves.  The true variance at a training point is about 1e-8; the
device computes 1e10 − Σv², a multiple of ulp(1e10) = 1.9e-6: each such variance is >= 0 or <= −1.9e-6, never in the clip band,
and which ones offend depends on the summation order.  No reference predicts that; the tests hold every call to the contract on
what it returns (contract()) and to the bars of tests/test_gpu_regimes.py against the float64 restatement, B = 8·cond·N·2⁻⁵³:
|Δμ| <= B(1 + max|μ|), |Δσ²| <= B·α² — 1e-2 at N = 1030 against the 1.9e-6 quantum: blind to rounding, open-eyed for a wrong
column or tile."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_program_cases as K  # noqa: E402

MAX_NEG_VAR = 1e-8
JITTER = 1e-18
FAR_BAR = 8 * 2.0 ** -52                                      # in units of α̃²


def flagged(u, v):            # squared exponential on all but the last coordinate, minus the product of the last ("flag") ones
    n = len(u) - 1
    return np.exp(-0.5 * sum((u[k] - v[k]) ** 2 for k in range(n))) - u[n] * v[n]


def clipped(var):
    var = np.asarray(var, float)
    return np.where((var < 0.0) & (var >= -MAX_NEG_VAR), 0.0, var)


def offenders(var):
    """Indices whose variance fails _clip_var (NaN counts, as in clip_var_kernel)."""
    var = np.asarray(var, float).reshape(-1)
    return np.flatnonzero(~(var >= -MAX_NEG_VAR))


def contract(api, rc, bad, var):
    """C1 and C2 on what one call returned; returns the offending indices.
    C1: rc == BOSS_E_NEG_VAR iff some returned var[j] < -1e-8 (or NaN), bad_index the smallest such j; else BOSS_OK and -1.
    C2: no returned entry lies in [-1e-8, 0)."""
    off = offenders(var)
    if off.size:
        assert rc == api.BOSS_E_NEG_VAR and bad == int(off[0]), (rc, bad, off[:8], np.asarray(var).reshape(-1)[off[:8]])
    else:
        assert rc == api.BOSS_OK and bad == -1, (rc, bad)
    v = np.asarray(var, float).reshape(-1)
    band = np.flatnonzero((v < 0.0) & (v >= -MAX_NEG_VAR))
    assert band.size == 0, (band[:8], v[band[:8]])
    return off


# ------------------------------------------------------------------------------------------ construction A
LAM_A = np.array([0.4, 0.6, 1.0])                             # spatial λ, flag λ
SIG_A = 0.05
FAR_X = 40.0
A_CASES = {
    # candidate index -> kind; every other candidate is "H".  The first offender is neither index 0 nor in the first tile of 32
    # (n20 has one tile), and an in-band far candidate follows it: the clip goes on behind an offender.
    "n20": dict(N=20, M=12, amp=1.0, kinds={1: -0.99e-8, 2: -5e-9, 3: 5e-9, 5: -1.01e-8, 6: -0.99e-8, 9: "P"}),
    "n130": dict(N=130, M=70, amp=1.0, kinds={1: -0.99e-8, 2: -5e-9, 3: 5e-9, 37: -2e-8, 38: -0.99e-8, 69: "P"}),
    "n130b": dict(N=130, M=16389, amp=1.0, kinds={1: -0.99e-8, 2: -5e-9, 3: 5e-9, 9000: "P", 9001: -0.99e-8, 16000: -5e-9,
                                                  16388: -1.01e-8}),
    "n130a3": dict(N=130, M=70, amp=3.0, kinds={1: -0.99e-8, 2: -5e-9, 3: 5e-9, 37: -1.01e-8, 38: -5e-9, 69: -2e-8}),
    "n1030": dict(N=1030, M=40, amp=1.0, kinds={1: -0.99e-8, 2: -5e-9, 3: 5e-9, 33: -1.01e-8, 34: -0.99e-8, 35: "P", 38: -2e-8}),
}
A_OFFENDERS = {"n20": [5, 9], "n130": [37, 69], "n130b": [9000, 16388], "n130a3": [37, 69], "n1030": [33, 35, 38]}
N1030_M3 = [0, 34, 33]                                       # columns of n1030 for the M <= 4 finish: H, in-band, offender


def far_flag(target, amp, lam_f=LAM_A[2]):
    """The flag coordinate at which a far candidate's variance is `target`: t² = 1 − target/α̃²."""
    return math.sqrt(1.0 - target / (amp + 1e-8) ** 2) * (lam_f + 1e-8)


class CaseA:
    """Inputs and expected values of one construction-A case.  Xs is the poisoned candidate set, Xs_clean the same with every
    offender replaced by the healthy candidate of its column.  want_* / bar_* per candidate (the poisoned set; *_clean likewise):
    the restatement with the project bars tol(1 + max|μ|), tol·max k(x*, x*) for H and P, the exact values for the far candidates."""

    def __init__(self, name):
        s = A_CASES[name]
        self.name, self.N, self.M, self.amp = name, s["N"], s["M"], s["amp"]
        self.lam, self.sig = LAM_A.copy(), SIG_A
        X2, y, Xs2 = K.data(2, self.N, self.M, seed=3)
        self.X = np.vstack([X2, np.zeros(self.N)])
        self.y = y
        self.kinds = ["H"] * self.M
        Xs = np.vstack([Xs2, np.zeros(self.M)])
        clean = Xs.copy()
        for j, kind in s["kinds"].items():
            self.kinds[j] = kind
            if kind == "P":
                Xs[2, j] = 1.5 * (self.lam[2] + 1e-8)
            else:
                Xs[:, j] = [FAR_X, FAR_X, far_flag(kind, self.amp)]
                if kind >= -MAX_NEG_VAR:
                    clean[:, j] = Xs[:, j]
        self.Xs, self.Xs_clean = Xs, clean
        self.ref = K.Restated(flagged, self.X, self.y, self.lam, self.amp, self.sig, Xs)
        self.a2 = self.ref.a2
        self.far = np.array([not isinstance(k, str) for k in self.kinds])
        self.off = [j for j, k in enumerate(self.kinds) if k == "P" or (not isinstance(k, str) and k < -MAX_NEG_VAR)]
        self.want_mu, self.want_var, self.bar_mu, self.bar_var = self._expected(self.ref.mu, self.ref.var, self.kinds)
        mu_c, var_c, _ = self.ref.predict(clean)
        self.kinds_clean = [k if j not in self.off else "H" for j, k in enumerate(self.kinds)]
        self.want_mu_clean, self.want_var_clean, self.bar_mu_clean, self.bar_var_clean = self._expected(mu_c, var_c, self.kinds_clean)
        for a in (self.X, self.y, self.Xs, self.Xs_clean, self.want_mu, self.want_var, self.bar_mu, self.bar_var, self.want_mu_clean,
                  self.want_var_clean, self.bar_mu_clean, self.bar_var_clean, self.ref.mu, self.ref.var, self.ref.kss):
            a.setflags(write=False)

    def _expected(self, mu, var, kinds):
        tol = self.ref.tol
        want_mu, want_var = mu.copy(), clipped(var)
        near = np.array([isinstance(k, str) for k in kinds])
        bar_mu = np.full(len(kinds), tol * (1 + np.abs(mu[near]).max()))
        bar_var = np.full(len(kinds), tol * self.a2)           # (max k(x*, x*) = α̃², at the healthy candidates)
        for j, k in enumerate(kinds):
            if isinstance(k, str):
                continue
            want_mu[j], bar_mu[j] = 0.0, 0.0
            in_band = -MAX_NEG_VAR <= k < 0.0
            want_var[j], bar_var[j] = (0.0, 0.0) if in_band else (k, FAR_BAR * self.a2)
        return want_mu, want_var, bar_mu, bar_var

    def columns(self, cols):
        """(Xs, want_mu, want_var, bar_mu, bar_var, offenders) of a sub-selection of the poisoned set."""
        cols = list(cols)
        off = [i for i, j in enumerate(cols) if j in self.off]
        return (np.asfortranarray(self.Xs[:, cols]), self.want_mu[cols], self.want_var[cols], self.bar_mu[cols], self.bar_var[cols], off)


_cases_a = {}


def case_a(name):
    if name not in _cases_a:
        _cases_a[name] = CaseA(name)
    return _cases_a[name]


# ------------------------------------------------------------------------------------------ construction B
N_MID = 37
LAM_B, AMP_B, SIG_B = np.array([3.0]), 1e5, 1e-4


class CaseB:
    def __init__(self, N, kernel, seed):
        rng = np.random.default_rng(seed)
        self.N, self.kernel, self.seed = N, kernel, seed
        self.X = (10.0 * np.arange(N) + rng.uniform(0.0, 4.0, N))[None, :]
        self.y = np.sin(self.X[0])
        self.Xs = np.concatenate([self.X[0, :N_MID] + 5.0, self.X[0]])[None, :]
        self.M = N_MID + N
        self.lam, self.amp, self.sig = LAM_B.copy(), AMP_B, SIG_B
        self.ref = K.Restated(K.BUILTIN[kernel], self.X, self.y, self.lam, self.amp, self.sig, self.Xs)
        self.a2 = self.ref.a2
        self.B = 8 * self.ref.cond * N * 2.0 ** -53
        self.mid = np.arange(self.M) < N_MID
        for a in (self.X, self.y, self.Xs, self.ref.mu, self.ref.var):
            a.setflags(write=False)

    def bars(self, mu, var, cols=None):
        """C3: (|Δμ| / bar, |Δσ²| / bar) against the float64 restatement; cols: the candidates the call was given."""
        cols = np.arange(self.M) if cols is None else np.asarray(cols)
        e_mu = np.abs(mu - self.ref.mu[cols]).max() / (self.B * (1 + np.abs(self.ref.mu[cols]).max()))
        e_var = np.abs(var - clipped(self.ref.var[cols])).max() / (self.B * self.a2)
        return float(e_mu), float(e_var)


_cases_b = {}


def case_b(N, kernel="matern52", seed=1):
    if (N, kernel, seed) not in _cases_b:
        _cases_b[(N, kernel, seed)] = CaseB(N, kernel, seed)
    return _cases_b[(N, kernel, seed)]


# ------------------------------------------------------------------------------------------ the C entry points, unwrapped
def _cols(api, Xs):
    Xs = api._f64(Xs)
    return api._f64(Xs.reshape(-1, 1)) if Xs.ndim == 1 else Xs


def predict_raw(api, g, Xs, mean_Xs=None):
    """boss_gp_predict -> (rc, bad_index, mu, var); the arrays start as NaN, so an entry the call did not write shows."""
    Xs = _cols(api, Xs)
    M = Xs.shape[1]
    ms = None if mean_Xs is None else api._f64(np.asarray(mean_Xs).reshape(-1), 1)
    mu, var, bad = np.full(M, np.nan), np.full(M, np.nan), C.c_long(-7)
    rc = api.load_library().boss_gp_predict(g._h, M, api._dp(Xs), api._dp(ms), api._dp(mu), api._dp(var), C.byref(bad))
    return rc, bad.value, mu, var


def predict_grad_raw(api, g, Xs):
    """boss_gp_predict_grad -> (rc, bad_index, mu, var, dmu, dvar)."""
    Xs = _cols(api, Xs)
    d, M = Xs.shape
    mu, var, bad = np.full(M, np.nan), np.full(M, np.nan), C.c_long(-7)
    dmu, dvar = np.full((d, M), np.nan, order="F"), np.full((d, M), np.nan, order="F")
    rc = api.load_library().boss_gp_predict_grad(g._h, M, api._dp(Xs), None, None, api._dp(mu), api._dp(var), api._dp(dmu), api._dp(dvar),
                                                 C.byref(bad))
    return rc, bad.value, mu, var, dmu, dvar


def predict_cov_raw(api, g, Xs):
    """boss_gp_predict_cov -> (rc, bad_index, mu, cov)."""
    Xs = _cols(api, Xs)
    M = Xs.shape[1]
    mu, cov, bad = np.full(M, np.nan), np.full((M, M), np.nan, order="F"), C.c_long(-7)
    rc = api.load_library().boss_gp_predict_cov(g._h, M, api._dp(Xs), None, api._dp(mu), api._dp(cov), C.byref(bad))
    return rc, bad.value, mu, cov


def warp_predict_raw(api, warp, g, Xs, grad=False):
    """boss_warp_predict[_grad] at P = S = 1 -> (rc, bad_index, mu, var[, dmu, dvar]) (dmu, dvar [M][d_user])."""
    Xs = _cols(api, Xs)
    du, M = Xs.shape
    arr = (C.c_void_p * 1)(g._h)
    mu, var, bad = np.full(M, np.nan), np.full(M, np.nan), C.c_long(-7)
    lib = api.load_library()
    if not grad:
        rc = lib.boss_warp_predict(warp._h, 1, 1, arr, M, api._dp(Xs), None, api._dp(mu), api._dp(var), C.byref(bad))
        return rc, bad.value, mu, var
    dmu, dvar = np.full((M, du), np.nan), np.full((M, du), np.nan)
    rc = lib.boss_warp_predict_grad(warp._h, 1, 1, arr, M, api._dp(Xs), None, None, api._dp(mu), api._dp(var), api._dp(dmu), api._dp(dvar),
                                    C.byref(bad))
    return rc, bad.value, mu, var, dmu, dvar
