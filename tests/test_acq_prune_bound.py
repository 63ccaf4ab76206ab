"""The bound behind the arg-max-only acquisition path (csrc/host_prune.inc), restated in numpy against the oracle.

EI is non-decreasing in σ and in c·μ − best, and the variance after the first s 256-row blocks of the forward substitution is the
posterior variance given the first 256·s observations, an upper bound on the final one.  So
    ub = EI(c·μ − best + δμ, c²(σ²_s + δv))
bounds every candidate's EI, and finishing the K largest bounds exactly, then whatever cannot be excluded by their maximum,
returns the oracle's first-index arg-max.  No GPU needed."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gp_oracle as O

KMU, KVAR = 1.2e-4, 1e-10           # PRUNE_KMU, PRUNE_KVAR of csrc/host_prune.inc
SHAPES = [(1100, 3, 4200), (1536, 6, 2100), (1024, 8, 8192)]
SEEDS = [0, 1, 2, 3]


def _problem(N, d, M, seed):
    rng = np.random.default_rng(100 + seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = np.random.default_rng(200 + seed).uniform(0, 1, (d, M))
    return X, y, Xs


_cache = {}


def _moments(N, d, M, seed):
    """(y, μ, exact σ², {s: σ²_s}) of one problem: computed once, shared by every case of it."""
    key = (N, d, M, seed)
    if key not in _cache:
        X, y, Xs = _problem(N, d, M, seed)
        post = O.gp_fit(X, y, "matern52", np.full(d, 0.5), 1.0, 0.05)
        Ks = O.kernelmatrix(post.h, post.X, Xs)
        V = sla.solve_triangular(post.L, Ks, lower=True, check_finite=False)
        mu = Ks.T @ post.a
        amp2 = post.h.amplitude ** 2
        sq = np.cumsum(V * V, axis=0)
        var = amp2 - sq[-1] + O.PREDICT_JITTER
        head = {s: amp2 - sq[256 * s - 1] + O.PREDICT_JITTER for s in (1, 2)}
        mu_o, var_o = O.gp_mean_and_var(post, Xs, clip=False)
        assert np.allclose(mu, mu_o, rtol=0, atol=1e-10) and np.allclose(var, var_o, rtol=0, atol=1e-10)
        _cache[key] = (y, mu, var, head, amp2)
    return _cache[key]


def _bound(mu, var_s, best, amp2, c=1.0):
    muf = c * mu
    dmu = KMU * (np.abs(muf) + abs(best) + abs(c) * np.sqrt(amp2))
    v = np.where(var_s < 0.0, 0.0, var_s) + KVAR * amp2
    sf = np.sqrt(c * c * v)
    diff = muf - best + dmu
    with np.errstate(divide="ignore", invalid="ignore"):
        z = diff / sf
        ei = diff * O.normcdf(z) + sf * O.normpdf(z)
    return np.where((diff == 0.0) & (sf == 0.0), 0.0, ei)


def _two_rounds(ub, exact, K):
    """index the device path returns, and how many candidates each round finished"""
    order = np.lexsort((np.arange(ub.size), -ub))              # largest bound first, ties by index
    sel = np.sort(order[:K])
    T = exact[sel].max()
    rest = np.ones(ub.size, dtype=bool)
    rest[sel] = False
    surv = np.flatnonzero(rest & ~(ub < T))
    alive = np.concatenate([sel, surv])
    return int(alive[O.argmax_first(exact[alive])]), sel.size, surv.size


@pytest.mark.parametrize("N,d,M", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_bound_holds_and_two_rounds_find_the_argmax(N, d, M, seed):
    y, mu, var, head, amp2 = _moments(N, d, M, seed)
    for best in (float(y.max()), float(y.max()) + 1.0, float(np.median(y))):
        exact = O.expected_improvement_lin([1.0], mu[None], O.clip_var(var)[None], best)
        want = int(O.argmax_first(exact))
        for s in (1, 2):
            assert np.all(head[s] >= var - 1e-14), "the head variance is an upper bound on the final one"
            ub = _bound(mu, head[s], best, amp2)
            worst = float(np.min(ub - exact))
            assert np.all(ub >= exact), (N, d, M, seed, best, s, worst)
            got, n1, n2 = _two_rounds(ub, exact, 64)
            print(f"N={N} d={d} M={M} seed={seed} best={best:.3f} s={s}: round 1 {n1}, round 2 {n2}, min(ub - exact) {worst:.3e}")
            assert got == want, (N, d, M, seed, best, s, got, want)


def test_bound_with_a_negative_fitness_coefficient():
    """c < 0: EI of the fitness c·y is still non-decreasing in σ = |c|·σ_y and in c·μ − best"""
    y, mu, var, head, amp2 = _moments(*SHAPES[0], 0)
    best = float((-y).max())
    exact = O.expected_improvement_lin([-1.0], mu[None], O.clip_var(var)[None], best)
    for s in (1, 2):
        ub = _bound(mu, head[s], best, amp2, c=-1.0)
        assert np.all(ub >= exact)
        assert _two_rounds(ub, exact, 64)[0] == int(O.argmax_first(exact))
