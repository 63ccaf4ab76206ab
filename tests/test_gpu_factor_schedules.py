"""The Cholesky update under the resident panel chain, on the device (pytest -m gpu): the deferred trailing schedule
(BOSS_CHAIN_TRAIL=4, the default from 16 to 64 block columns: trail_plan / potrf_colupd_tab_kernel) and its neighbours.

  (a) whole factors against a float64 reference across the chain's size range — both batch depths of the deferred schedule
      (P, Q = 2, 1 up to 44 block columns, 4, 3 from 46 on), its lower edge (1792 rows: 14 block columns, mode 0) and the first
      size past the chain (8193 rows) — checked tile by tile, so that a panel skipped or applied twice names its tile;
  (b) bit-identity of the factor across the trailing schedules and batch settings, each in a process of its own (the schedule
      switches are read once per process);
  (c) the gradient-observation, nonstationary and semiparametric models under the deferred schedule;
  (d) failures under the chain: a pivot failure deep in the factor, non-finite data, and several sizes interleaved on one context.

Every update asserts what actually ran (boss_debug_update_path): the chain, the trailing schedule, no fallback — a test that
landed on the gate schedule would otherwise pass without exercising the deferred one."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK = 128
CHILD_TIMEOUT = 300


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


def want_path(Nrows, trail_env=None):
    """(chained, trail mode) the library takes for a factor of Nrows rows (Np = round_up(N, 256), BOSS_CHAIN_NP_MAX = 8192)."""
    Np = -(-Nrows // 256) * 256
    if Np > 8192:
        return 0, -1
    if trail_env is not None:
        return 1, trail_env
    return 1, 0 if Np // BLK < 16 else 4


def check_path(api, g, Nrows, fb0, trail_env=None, tag=""):
    ch, mode, fell = api._update_path(g)
    n, off = api._fallbacks(0)
    assert (ch, mode) == want_path(Nrows, trail_env), f"{tag} N={Nrows}: chained={ch} trail_mode={mode}"
    assert fell == 0 and n == fb0 and off == 0, f"{tag} N={Nrows}: fell_back={fell}, fallbacks {fb0} -> {n}, chain_off={off}"


def make(d, N, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    return X, y


def factor_hash(L, z):
    h = hashlib.sha256(np.ascontiguousarray(L).tobytes())
    h.update(np.ascontiguousarray(z).tobytes())
    return h.hexdigest()


def rcond(L, K):
    """Reciprocal 1-norm condition number of K from its Cholesky factor (LAPACK dpocon, O(N²))."""
    from scipy.linalg import lapack
    rc, info = lapack.dpocon(np.asfortranarray(L), np.abs(K).sum(0).max(), uplo="L")
    assert info == 0
    return rc


def tile_residuals(L, K):
    """max |L Lᵀ − K| of every lower 128×128 tile: {(i, j): value}."""
    N = K.shape[0]
    nt = -(-N // BLK)
    out = {}
    for i in range(nt):
        r0, r1 = i * BLK, min(N, (i + 1) * BLK)
        R = np.abs(L[r0:r1, :r1] @ L[:r1, :r1].T - K[r0:r1, :r1])
        for j in range(i + 1):
            out[(i, j)] = float(R[:, j * BLK:min(r1, (j + 1) * BLK)].max())
    return out


def check_factor(L, z, y, lp, K, post_logpdf, N, tag, cond_aware=False):
    # the factor's shape: exactly lower triangular with a positive, finite diagonal
    assert not np.triu(L, 1).any(), f"{tag}: entries above the diagonal"
    dg = np.diag(L)
    assert np.all(np.isfinite(dg)) and dg.min() > 0.0, f"{tag}: diagonal not positive and finite"
    assert np.all(np.isfinite(L)), f"{tag}: non-finite factor entries"
    # L Lᵀ = K tile by tile, against the backward-stable bound ||LLᵀ − K|| <= c N eps ||K|| (test_full_size_properties)
    bound = 50 * N * 2.0 ** -53 * np.abs(K).max()
    res = tile_residuals(L, K)
    bad = sorted(((v, t) for t, v in res.items() if not v <= bound), reverse=True)
    assert not bad, f"{tag}: {len(bad)} tile(s) of LLᵀ − K over {bound:.3g}, worst (i, j) = " + \
        ", ".join(f"{t}: {v:.3g}" for v, t in bad[:6])
    # L z = y (componentwise backward error) and the log-likelihood identity
    atol = max(1e-10 * (1 + np.abs(y).max()), 8 * N * 2.0 ** -53 * (np.abs(L) @ np.abs(z)).max())
    assert np.abs(L @ z - y).max() <= atol, f"{tag}: L z != y"
    ident = -0.5 * (N * np.log(2 * np.pi) + 2 * np.log(dg).sum() + z @ z)
    assert abs(lp - ident) <= 1e-9 * (1 + abs(lp)), f"{tag}: logpdf {lp!r} against its factor {ident!r}"
    tol = 1e-9
    if cond_aware:                                             # the parity tests' condition-aware bound beyond cond(K) = 1e6
        tol = max(tol, N * 2.0 ** -53 * 8 / rcond(L, K))
    assert abs(lp - post_logpdf) <= tol * (1 + abs(post_logpdf)), f"{tag}: logpdf {lp!r} against LAPACK {post_logpdf!r} (tol {tol:.3g})"


# ------------------------------------------------------------------------------------------
# (a) size sweep against a float64 reference
# ------------------------------------------------------------------------------------------
SWEEP = [(N, "matern52", 0.5, 0.05) for N in (1792, 1793, 2048, 3000, 5632, 5633, 7000, 8192, 8193)] + \
        [(2048, "sqexp", 0.3, 1e-3), (5633, "sqexp", 0.3, 1e-3)]


@pytest.mark.parametrize("N,kernel,ls,sigma", SWEEP)
def test_factor_tiles_against_float64_reference(api, O, N, kernel, ls, sigma):
    """1792 rows: 14 block columns, mode 0; 1793 … 5632: 16 … 44 block columns, P, Q = 2, 1; 5633 … 8192: 46 … 64, P, Q = 4, 3;
    8193: past the chain.  The squared-exponential cases are ill-conditioned (σ = 1e-3: cond(K) ≈ 1e8 … 1e9)."""
    d = 8
    X, y = make(d, N, seed=N)
    lam = np.full(d, ls)
    fb0, _ = api._fallbacks(0)
    g = api.GP(X, y, kernel)
    lp = g.update(lam, 1.0, sigma)
    check_path(api, g, N, fb0, tag=kernel)
    L, z = g.factor()
    g.close()
    h = O.finite_gp_params(kernel, d, lam, 1.0, sigma)
    K = O.kernelmatrix(h, X)
    K[np.diag_indices(N)] += h.noise_std ** 2
    post = O.gp_fit(X, y, kernel, lam, 1.0, sigma)
    check_factor(L, z, y, lp, K, post.logpdf, N, f"N={N} {kernel} σ={sigma}", cond_aware=sigma < 0.01)


# ------------------------------------------------------------------------------------------
# (b) bit-identity across schedules, one process per schedule
# ------------------------------------------------------------------------------------------
CHILD = r"""
import hashlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from boss_jl_amd import api
api.load_library()
jobs = json.loads(sys.argv[2])
def make(d, N, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    return X, y
out = []
for job in jobs:
    kind, N, seed = job["kind"], job["N"], job["seed"]
    if kind == "gp":
        X, y = make(8, N, seed)
        g = api.GP(X, y, "matern52")
        lp = g.update(np.full(8, 0.5), 1.0, job.get("sigma", 0.05))
    else:
        g, lp = MODELS[kind](N, seed)
    L, z = g.factor()
    h = hashlib.sha256(np.ascontiguousarray(L).tobytes()); h.update(np.ascontiguousarray(z).tobytes())
    out.append({"N": N, "kind": kind, "lp": float(lp).hex(), "hash": h.hexdigest(), "path": list(api._update_path(g))})
    g.close()
    del L, z
print("RES " + json.dumps({"runs": out, "fallbacks": list(api._fallbacks(0))}))
"""


def run_child(env_extra, jobs, models=""):
    """Run `jobs` in a fresh process under the extra environment (one at a time, under a time limit); returns its report."""
    code = (models or "MODELS = {}\n") + CHILD
    env = dict(os.environ)
    for k in ("BOSS_CHAIN_TRAIL", "BOSS_TRAIL_PANELS", "BOSS_TRAIL_LAG"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code, ROOT, json.dumps(jobs)], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and "RES " in r.stdout, f"{env_extra}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    rep = json.loads(r.stdout.split("RES ", 1)[1].splitlines()[0])
    assert rep["fallbacks"] == [0, 0], f"{env_extra}: fallbacks / chain off {rep['fallbacks']}"
    return rep


SCHEDULES = [
    ("default", {}, None),
    ("mode 0", {"BOSS_CHAIN_TRAIL": "0"}, 0),
    ("mode 1", {"BOSS_CHAIN_TRAIL": "1"}, 1),
    ("mode 2", {"BOSS_CHAIN_TRAIL": "2"}, 2),
    ("P, Q = 1, 1", {"BOSS_TRAIL_PANELS": "1", "BOSS_TRAIL_LAG": "1"}, None),
    ("P, Q = 3, 2", {"BOSS_TRAIL_PANELS": "3", "BOSS_TRAIL_LAG": "2"}, None),
    ("P, Q = 8, 3", {"BOSS_TRAIL_PANELS": "8", "BOSS_TRAIL_LAG": "3"}, None),
]
B_SIZES = (2048, 5632, 5633, 8192)


def test_schedules_give_bit_identical_factors(api):
    """Every strip receives every earlier panel once, in ascending order, through the same MFMA sequence whichever launches
    group the panels (K = 128·npan in one pass of syrk_tile, exact ring tail), so the factor, z and the logpdf are the same
    bits under the per-step launches (0), the main-stream pairs (1), the two-stream gated schedule (2: bulk updates of
    64×128 tiles beside the chain, potrf_syrk_kernel, the same syrk_tile accumulation per element) and the deferred
    schedule at any batch depth.  A (strip, panel) pair dropped or applied twice by a plan breaks the equality at its size."""
    jobs = [{"kind": "gp", "N": N, "seed": 100 + N} for N in B_SIZES]
    reps = {}
    for name, env, mode in SCHEDULES:
        rep = run_child(env, jobs)
        for run in rep["runs"]:
            want = want_path(run["N"], mode)
            assert tuple(run["path"]) == (*want, 0), f"{name} N={run['N']}: path {run['path']}, want {want}"
        reps[name] = rep["runs"]
    base = reps["default"]
    for name, runs in reps.items():
        for a, b in zip(base, runs):
            assert (b["hash"], b["lp"]) == (a["hash"], a["lp"]), \
                f"N={a['N']} ({-(-a['N'] // 256) * 2} block columns): {name} differs from the default schedule"


# ------------------------------------------------------------------------------------------
# (c) the other models under the deferred schedule
# ------------------------------------------------------------------------------------------
MODEL_DEFS = r"""
import numpy as np
from boss_jl_amd import api as _api

def _ggp_data(N, seed):
    d = 8
    n = N // (1 + d)
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, n))
    y = np.sin(3 * X).sum(0) + 0.05 * rng.standard_normal(n)
    dY = 3 * np.cos(3 * X) + 0.1 * rng.standard_normal((d, n))
    return X, y, dY

def _ngp_data(N, seed):
    d = 3
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    lam = 0.25 + 0.1 * np.sin(2 * X) + 0.05 * X[::-1]
    amp = 1.0 + 0.3 * np.cos(3 * X[0])
    noi = 0.05 + 0.02 * X[1]
    return X, y, lam, amp, noi

def _semi_data(N, seed):
    d = 6
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    X[2] = rng.integers(0, 5, N) + 0.3 * rng.uniform(-1, 1, N)          # a discrete dimension (rounded by the model)
    disc = np.zeros(d, bool)
    disc[2] = True
    w = np.linspace(0.5, 1.5, d)
    m = 0.1 + 0.2 * (w @ X)
    y = m + np.sin(3 * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    return X, y, disc, m

def _ggp(N, seed):
    X, y, dY = _ggp_data(N, seed)
    g = _api.GradGP(X, y, dY, "matern52")
    return g, g.update(np.full(8, 0.6), 1.0, 0.05, 0.1)

def _ngp(N, seed):
    X, y, lam, amp, noi = _ngp_data(N, seed)
    g = _api.GibbsGP(X, y)
    return g, g.update(lam, amp, noi)

def _semi(N, seed):
    X, y, disc, m = _semi_data(N, seed)
    g = _api.GP(X, y, "matern52", discrete=disc)
    return g, g.update(np.linspace(0.4, 0.7, 6), 1.0, 0.05, mean_X=m)

MODELS = {"ggp": _ggp, "ngp": _ngp, "semi": _semi}
"""
MODEL_JOBS = [("ggp", 2700), ("ggp", 6300), ("ngp", 6000), ("semi", 5633)]


@pytest.fixture(scope="module")
def models(api):
    ns = {}
    exec(compile(MODEL_DEFS, "model_defs", "exec"), ns)
    return ns


def _child_models_code():
    return "import sys\nsys.path.insert(0, sys.argv[1])\n" + MODEL_DEFS


@pytest.mark.parametrize("kind,N", MODEL_JOBS)
def test_other_models_under_the_deferred_schedule(api, O, models, kind, N):
    """GGP at 2700 (22 block columns, P = 2) and 6300 augmented rows (50, P = 4), NGP at 6000 rows, a semiparametric mean with a
    discrete dimension at 5633 rows: factor and logpdf against the oracle at the parity tests' tolerances."""
    seed = 7 + N
    fb0, _ = api._fallbacks(0)
    g, lp = models["MODELS"][kind](N, seed)
    check_path(api, g, g.N, fb0, tag=kind)
    L, z = g.factor()
    g.close()
    if kind == "ggp":
        X, y, dY = models["_ggp_data"](N, seed)
        post = O.gradient_gp_fit(X, y, dY, "matern52", np.full(8, 0.6), 1.0, 0.05, 0.1)
        Lo = post.L
    elif kind == "ngp":
        X, y, lam, amp, noi = models["_ngp_data"](N, seed)
        post = O.nonstationary_fit(X, y, lam, amp, noi)
        Lo = post.L
    else:
        X, y, disc, m = models["_semi_data"](N, seed)
        post = O.gp_fit(X, y, "matern52", np.linspace(0.4, 0.7, 6), 1.0, 0.05, mean=m, discrete=disc)
        Lo = post.L
    Nr = Lo.shape[0]
    K = Lo @ Lo.T
    tol = max(1e-9, Nr * 2.0 ** -53 * 8 / rcond(Lo, K))       # test_gradient_gp_parity's cond(K)·N·2⁻⁵³·8
    assert L.shape == Lo.shape and np.all(np.diag(L) > 0) and not np.triu(L, 1).any()
    assert abs(lp - post.logpdf) <= tol * (1 + abs(post.logpdf)), f"{kind} N={Nr}: logpdf {lp!r} against {post.logpdf!r}"
    assert np.abs(L - Lo).max() <= tol * np.abs(Lo).max(), f"{kind} N={Nr}: factor differs from LAPACK's by {np.abs(L - Lo).max():.3g}"


def test_other_models_bit_identical_to_mode_0(api):
    jobs = [{"kind": k, "N": N, "seed": 7 + N} for k, N in MODEL_JOBS]
    code = _child_models_code()
    a = run_child({}, jobs, models=code)
    b = run_child({"BOSS_CHAIN_TRAIL": "0"}, jobs, models=code)
    for ra, rb in zip(a["runs"], b["runs"]):
        assert tuple(ra["path"]) == (*want_path(ra["N"]), 0), ra
        assert rb["path"] == [1, 0, 0], rb
        assert (ra["hash"], ra["lp"]) == (rb["hash"], rb["lp"]), f"{ra['kind']} N={ra['N']}: deferred schedule differs from mode 0"


# ------------------------------------------------------------------------------------------
# (d) failures under the chain
# ------------------------------------------------------------------------------------------
def pivot_of(exc):
    m = re.search(r"pivot (-?\d+) failed", str(exc))
    assert m, str(exc)
    return int(m.group(1))


def clean_update(api, X, y, fb0, tag):
    g = api.GP(X, y, "matern52")
    g.update(np.full(X.shape[0], 0.5), 1.0, 0.05)
    check_path(api, g, X.shape[1], fb0, tag=tag)
    L, z = g.factor()
    g.close()
    return factor_hash(L, z)


def test_deep_pivot_failure_leaves_the_chain_consistent(api, O):
    """4096 rows (32 block columns, mode 4): 3000 well-separated points and 1096 copies of one point at noise 0 — the copies'
    eliminated pivots are rounding noise, so the factorisation fails a few columns past the first copy, deep in the chain."""
    from scipy.linalg import lapack
    d, N, c0 = 8, 4096, 3000
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (d, N))
    X[:, c0:] = rng.uniform(0, 1, (d, 1))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d)
    lam = np.full(d, 0.01)
    fb0, _ = api._fallbacks(0)
    g = api.GP(X, y, "matern52")
    with pytest.raises(api.PosDefException) as ei:
        g.update(lam, 1.0, 0.0)
    piv = pivot_of(ei.value)                                  # 1-based failed column
    check_path(api, g, N, fb0, tag="failed update")
    h = O.finite_gp_params("matern52", d, lam, 1.0, 0.0)
    K = O.kernelmatrix(h, X)
    K[np.diag_indices(N)] += h.noise_std ** 2
    _, info = lapack.dpotrf(K, lower=1)
    assert info > c0 and piv > c0, (piv, info)
    assert (piv - 1) // BLK == (info - 1) // BLK, f"device fails at column {piv}, LAPACK at {info}"
    with pytest.raises(api.BossError):                        # the handle is unfitted
        g.factor()
    # the next update on the same handle (sequence words of the context consistent) equals a fresh handle's
    g.update(np.full(d, 0.5), 1.0, 0.05)
    check_path(api, g, N, fb0, tag="after the failure")
    L, z = g.factor()
    g.close()
    assert factor_hash(L, z) == clean_update(api, X, y, fb0, "fresh handle")


def test_non_finite_data_under_the_chain(api, O):
    """NaN in X (column 3000: the first NaN pivot, where LAPACK's dpotrf2 stops), NaN and ±Inf in y (a non-finite likelihood): each a
    PosDefException, no wait that gives up, the chain stays on, and a clean update afterwards is unchanged."""
    from scipy.linalg import lapack
    d, N, c = 8, 4096, 3000
    X, y = make(d, N, seed=21)
    lam = np.full(d, 0.5)
    fb0, _ = api._fallbacks(0)
    ref = clean_update(api, X, y, fb0, "reference")
    Xn = X.copy()
    Xn[3, c] = np.nan
    h = O.finite_gp_params("matern52", d, lam, 1.0, 0.05)
    K = O.kernelmatrix(h, Xn)
    K[np.diag_indices(N)] += h.noise_std ** 2
    # (the host's dpotrf need not test its pivots for NaN: the first non-finite pivot is column c + 1 because the leading c
    # columns factor and row c of K is NaN)
    assert lapack.dpotrf(K[:c, :c], lower=1)[1] == 0 and np.isnan(K[c, c])
    info = c + 1
    g = api.GP(Xn, y, "matern52")
    with pytest.raises(api.PosDefException) as ei:
        g.update(lam, 1.0, 0.05)
    assert pivot_of(ei.value) == info
    check_path(api, g, N, fb0, tag="NaN in X")
    g.close()
    assert clean_update(api, X, y, fb0, "after NaN in X") == ref
    g = api.GP(X, y, "matern52")
    for bad in (np.nan, np.inf, -np.inf):
        yb = y.copy()
        yb[c] = bad
        g.set_y(yb)
        with pytest.raises(api.PosDefException):
            g.update(lam, 1.0, 0.05)
        check_path(api, g, N, fb0, tag=f"y = {bad}")
        with pytest.raises(api.BossError):
            g.factor()
    g.set_y(y)                                               # the same handle, clean again
    g.update(lam, 1.0, 0.05)
    check_path(api, g, N, fb0, tag="y clean again")
    L, z = g.factor()
    g.close()
    assert factor_hash(L, z) == ref


ALL_ONES_CHILD = r"""
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from boss_jl_amd import api
api.load_library()
d, N, c = 8, 4096, 3000
rng = np.random.default_rng(21)
X = rng.uniform(0, 1, (d, N))
y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
X[3, c] = np.frombuffer(b"\xff" * 8)[0]                   # a NaN whose bits are all ones: the strips' "not written yet" pattern
g = api.GP(X, y, "matern52")
t0 = time.perf_counter()
try:
    g.update(np.full(d, 0.5), 1.0, 0.05)
    err = ""
except api.BossError as e:
    err = type(e).__name__ + ": " + str(e)
ms = 1e3 * (time.perf_counter() - t0)
print("RES " + json.dumps({"err": err, "ms": ms, "path": list(api._update_path(g)), "fallbacks": list(api._fallbacks(0))}))
"""


def test_all_ones_nan_is_not_taken_for_a_missing_inverse(api):
    """The resident strips poll inv16 for the all-ones bit pattern ("not written yet", follow_strip in chain.hpp).  A NaN input
    with exactly those bits keeps its payload through the Gram and the pivot chain; stored as it is it made the pollers spin until
    their budget ran out, and gp_finish then switched the chain off for the rest of the process.  inv16 entries go out as the
    canonical quiet NaN (inv16_entry, potrf.hpp): the update fails like any NaN pivot, the chain stays on.  Once, in a child."""
    r = subprocess.run([sys.executable, "-c", ALL_ONES_CHILD, ROOT], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and "RES " in r.stdout, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    rep = json.loads(r.stdout.split("RES ", 1)[1].splitlines()[0])
    assert rep["err"].startswith("PosDefException") and "pivot 3001 failed" in rep["err"], rep
    assert rep["path"] == [1, 4, 0] and rep["fallbacks"] == [0, 0], rep


INTERLEAVED = [("A", "gp", 4096), ("B", "gp", 6000), ("C", "gp", 2048), ("D", "ngp", 3000)]


def test_interleaved_sizes_on_one_context(api, models):
    """Four handles of four sizes (four work tables, the chain's and the critical strips' sequence words advancing by different
    amounts) updated in the order A B A C D B A on one context: every update equals that handle's update in a process of its own."""
    code = _child_models_code()
    want = {}
    for name, kind, N in INTERLEAVED:
        rep = run_child({}, [{"kind": kind, "N": N, "seed": 300 + N}], models=code)
        want[name] = rep["runs"][0]
    fb0, _ = api._fallbacks(0)
    handles = {}
    for name, kind, N in INTERLEAVED:
        if kind == "gp":
            X, y = make(8, N, 300 + N)
            handles[name] = (api.GP(X, y, "matern52"), lambda g: g.update(np.full(8, 0.5), 1.0, 0.05))
        else:
            X, y, lam, amp, noi = models["_ngp_data"](N, 300 + N)
            handles[name] = (api.GibbsGP(X, y), lambda g, lam=lam, amp=amp, noi=noi: g.update(lam, amp, noi))
    for step, name in enumerate("ABACDBA"):
        g, upd = handles[name]
        lp = upd(g)
        check_path(api, g, g.N, fb0, tag=f"step {step} ({name})")
        L, z = g.factor()
        assert (factor_hash(L, z), float(lp).hex()) == (want[name]["hash"], want[name]["lp"]), \
            f"step {step}: handle {name} (N = {g.N}) differs from its update in a process of its own"
    for g, _ in handles.values():
        g.close()
