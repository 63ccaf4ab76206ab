"""Shared by tests/test_kernel_program_host.py and tests/test_gpu_kernel_program.py: the covariance closures a DeviceKernel is traced
from, and the numpy/scipy restatement of a program-kernel posterior (the conventions of include/bosship.h, boss_kgp_create).

Every closure f(u, v) works on traced vectors and on numpy arrays alike; written with index loops, it also broadcasts over
u[k] of shape (N, 1) against v[k] of shape (1, M), which is how `gram` evaluates whole matrices with the closure itself.  The
dot-product closure is spelled `u @ v + 1` (what a user writes); its matrix forms in `gram` / `pairs` are held to the closure pair by pair
in the host test."""
import math

import numpy as np
import scipy.linalg as sla

PERIOD = 1.7                                                  # of the periodic factor, in scaled coordinates


def _r2(u, v):
    return sum((u[k] - v[k]) ** 2 for k in range(len(u)))


def expo(u, v):                                               # exponential = Matérn-1/2
    return np.exp(-np.sqrt(_r2(u, v)))


def ratquad(u, v):                                            # rational quadratic, shape 2.0
    return (1 + _r2(u, v) / (2 * 2.0)) ** -2.0


def persq(u, v):                                              # periodic in the first coordinate × squared exponential
    return np.exp(-2.0 * np.sin(math.pi * (u[0] - v[0]) / PERIOD) ** 2) * np.exp(-0.5 * _r2(u, v))


def dot1(u, v):                                               # dot product plus a constant: k(x, x) differs from point to point
    return u @ v + 1


def matern52(u, v):
    r2 = _r2(u, v)
    s = np.sqrt(5.0 * r2)
    return (1 + s + 5.0 / 3.0 * r2) * np.exp(-s)


def matern32(u, v):
    s = np.sqrt(3.0 * _r2(u, v))
    return (1 + s) * np.exp(-s)


def sqexp(u, v):
    return np.exp(-0.5 * _r2(u, v))


CLOSURES = {"expo": expo, "ratquad": ratquad, "persq": persq, "dot1": dot1, "matern52": matern52}
BUILTIN = {"matern32": matern32, "matern52": matern52, "sqexp": sqexp}


def gram(f, U, V):
    """f(U[:, i], V[:, j]) for all pairs: N×M."""
    if f is dot1:
        return U.T @ V + 1                                    # (`@` does not broadcast the way the index loops do)
    d = U.shape[0]
    with np.errstate(all="ignore"):
        return np.asarray(f([U[k][:, None] for k in range(d)], [V[k][None, :] for k in range(d)]), float)


def pairs(f, U, V):
    """f(U[:, j], V[:, j]) for every column j, evaluated by the closure on whole rows at once."""
    if f is dot1:
        return (U * V).sum(0) + 1
    d = U.shape[0]
    with np.errstate(all="ignore"):
        return np.asarray(f([U[k] for k in range(d)], [V[k] for k in range(d)]), float) + np.zeros(U.shape[1])


def data(d, N, M, seed=1, scale=None):
    """Points in [0, 1]^d (dimension k stretched by scale[k]), a smooth target with noise, M candidates."""
    rng = np.random.default_rng(seed)
    sc = np.ones(d) if scale is None else np.asarray(scale, float)
    X = rng.uniform(0, 1, (d, N)) * sc[:, None]
    y = np.sin(2 * np.pi * X / sc[:, None]).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = np.random.default_rng(seed + 1000).uniform(0, 1, (d, M)) * sc[:, None]
    return X, y, Xs


class Restated:
    """K from the closure, scipy.linalg.cholesky, then solves: logpdf, μ, σ² (unclipped), k(x*, x*), cond(K), tol."""

    def __init__(self, f, X, y, lam, amp, sig, Xs=None, discrete=None, mean_X=None, mean_Xs=None, want_cond=True):
        d, N = X.shape
        lamp = np.asarray(lam, float) + 1e-8
        self.a2, self.s2 = (amp + 1e-8) ** 2, (sig + 1e-8) ** 2
        disc = np.zeros(d, bool) if discrete is None else np.asarray(discrete, bool)
        self.scaled = lambda Z: np.where(disc[:, None], np.rint(Z), Z) / lamp[:, None]   # np.rint: half to even, as Julia's round
        self.f = f
        self.U = self.scaled(np.asarray(X, float))
        K = self.a2 * gram(f, self.U, self.U)
        K[np.diag_indices(N)] += self.s2
        self.K = K
        self.cond = float(np.linalg.cond(K)) if want_cond else float("nan")
        self.tol = max(1e-9, self.cond * N * 2.0 ** -53 * 8)
        self.L = sla.cholesky(K, lower=True, check_finite=False)
        delta = np.asarray(y, float) - (0.0 if mean_X is None else np.asarray(mean_X, float))
        self.z = sla.solve_triangular(self.L, delta, lower=True, check_finite=False)
        self.a = sla.solve_triangular(self.L, self.z, lower=True, trans="T", check_finite=False)
        self.logpdf = -0.5 * (N * math.log(2.0 * math.pi) + 2.0 * float(np.log(np.diag(self.L)).sum()) + float(self.z @ self.z))
        if Xs is not None:
            self.mu, self.var, self.kss = self.predict(Xs, mean_Xs)

    def predict(self, Xs, mean_Xs=None):
        Us = self.scaled(np.asarray(Xs, float))
        Ks = self.a2 * gram(self.f, self.U, Us)
        mu = (0.0 if mean_Xs is None else np.asarray(mean_Xs, float)) + Ks.T @ self.a
        V = sla.solve_triangular(self.L, Ks, lower=True, check_finite=False)
        kss = self.a2 * pairs(self.f, Us, Us)
        var = kss - (V * V).sum(0) + 1e-18
        return mu, var, kss
