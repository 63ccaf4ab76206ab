"""Shared by tests/test_kernel_grad_host.py and tests/test_gpu_kernel_grad.py: closed-form partial derivatives of the covariance
closures of kernel_program_cases, and the numpy/scipy restatement of a program-kernel posterior's gradients built on them.

Partials are taken in the scaled coordinates the closures see: PARTIALS[name](U, V) -> (∂f/∂u, ∂f/∂v), each of the broadcast shape
of U and V (leading axis d).  At r = 0 the stationary kernels give 0: the true derivative of the Matérn and smooth kernels, and for
the exponential kernel the 0 KernelFunctions / Distances return at its cusp.

RestatedGrad adds to kernel_program_cases.Restated, with K⁻¹, W = K⁻¹K* from plain scipy solves and 1/λ_m short for 1/(λ_m+1e-8):
    ∂logpdf/∂θ = ½ Σ_ij G_ij ∂K_ij/∂θ ,  G = a aᵀ − K⁻¹ ,
    ∂K_ij/∂λ_m = −α² (f_u,m(u_i, u_j) u_i,m + f_v,m(u_i, u_j) u_j,m)/λ_m ,  ∂K/∂α = 2(α+1e-8) F ,  ∂K/∂σ = 2(σ+1e-8) I ;
    ∇μ_m(x*)  = ∇m_m + (1/λ_m) Σ_i a_i α² f_v,m(u_i, u*) ,
    ∇σ²_m(x*) = (1/λ_m) [α² (f_u,m + f_v,m)(u*, u*) − 2 Σ_i W_i α² f_v,m(u_i, u*)] ,
the kernel parts 0 in discrete dimensions (they are rounded inside the kernel)."""
import math

import numpy as np
import scipy.linalg as sla

import kernel_program_cases as cases

ALL = dict(cases.CLOSURES, **cases.BUILTIN)                  # expo, ratquad, persq, dot1, matern52, matern32, sqexp
STATIONARY = sorted(set(ALL) - {"dot1"})


def _delta(U, V):
    D = np.asarray(U, float) - np.asarray(V, float)
    return D, (D * D).sum(0)


def _stationary(scale_of_r2):
    """f depends on Δ = u − v alone: ∂f/∂u = c(Δ)·Δ (+ extra), ∂f/∂v = −∂f/∂u."""
    def partials(U, V):
        D, r2 = _delta(U, V)
        with np.errstate(all="ignore"):
            gu = scale_of_r2(D, r2)
        return gu, -gu
    return partials


def _d_expo(D, r2):
    r = np.sqrt(r2)
    return np.where(r2 > 0, -np.exp(-r) * D / np.where(r2 > 0, r, 1.0), 0.0)


def _d_ratquad(D, r2):
    return -(1 + r2 / 4.0) ** -3.0 * D


def _d_persq(D, r2):
    f = np.exp(-2.0 * np.sin(math.pi * D[0] / cases.PERIOD) ** 2) * np.exp(-0.5 * r2)
    g = -f * D
    g[0] = g[0] - f * (2.0 * math.pi / cases.PERIOD) * np.sin(2.0 * math.pi * D[0] / cases.PERIOD)
    return g


def _d_matern52(D, r2):
    s = np.sqrt(5.0 * r2)
    return -(5.0 / 3.0) * (1 + s) * np.exp(-s) * D


def _d_matern32(D, r2):
    return -3.0 * np.exp(-np.sqrt(3.0 * r2)) * D


def _d_sqexp(D, r2):
    return -np.exp(-0.5 * r2) * D


def _d_dot1(U, V):
    U, V = np.broadcast_arrays(np.asarray(U, float), np.asarray(V, float))
    return V.copy(), U.copy()


PARTIALS = {"expo": _stationary(_d_expo), "ratquad": _stationary(_d_ratquad), "persq": _stationary(_d_persq), "dot1": _d_dot1,
            "matern52": _stationary(_d_matern52), "matern32": _stationary(_d_matern32), "sqexp": _stationary(_d_sqexp)}


def name_of(f):
    return next(n for n, g in ALL.items() if g is f)


def fd_partials(f, U, V, h=1e-5):
    """Central differences of the closure itself, pair by pair: (∂f/∂u, ∂f/∂v), d×n each."""
    d, n = U.shape
    out = np.zeros((2, d, n))
    for side in range(2):
        for m in range(d):
            P, Q = [U.copy(), V.copy()], [U.copy(), V.copy()]
            P[side][m] += h
            Q[side][m] -= h
            out[side, m] = (cases.pairs(f, *P) - cases.pairs(f, *Q)) / (2 * h)
    return out[0], out[1]


class RestatedGrad(cases.Restated):
    """Restated plus ∂logpdf/∂(λ, α, σ) (`dlogpdf`, d + 2 entries) and, at candidates, ∇μ, ∇σ² (d×M each)."""

    def __init__(self, f, X, y, lam, amp, sig, Xs=None, discrete=None, mean_X=None, mean_Xs=None, mean_grad=None, want_cond=True):
        super().__init__(f, X, y, lam, amp, sig, Xs, discrete, mean_X, mean_Xs, want_cond)
        d, N = np.asarray(X).shape
        self.partials = PARTIALS[name_of(f)]
        self.lamp = np.asarray(lam, float) + 1e-8
        self.disc = np.zeros(d, bool) if discrete is None else np.asarray(discrete, bool)
        self.Kinv = sla.cho_solve((self.L, True), np.eye(N), check_finite=False)
        G = np.outer(self.a, self.a) - self.Kinv
        Fu, Fv = self.partials(self.U[:, :, None], self.U[:, None, :])          # d×N×N
        dK = -self.a2 * (Fu * self.U[:, :, None] + Fv * self.U[:, None, :]) / self.lamp[:, None, None]
        F = (self.K - self.s2 * np.eye(N)) / self.a2
        self.dlogpdf = np.concatenate([0.5 * (G[None] * dK).sum((1, 2)), [0.5 * (G * F).sum() * 2.0 * (amp + 1e-8),
                                                                         0.5 * np.trace(G) * 2.0 * (sig + 1e-8)]])
        if Xs is not None:
            self.dmu, self.dvar = self.predict_grad(Xs, mean_grad)

    def predict_grad(self, Xs, mean_grad=None):
        Us = self.scaled(np.asarray(Xs, float))
        Ks = self.a2 * cases.gram(self.f, self.U, Us)
        W = sla.cho_solve((self.L, True), Ks, check_finite=False)             # K⁻¹ K*
        _, Fv = self.partials(self.U[:, :, None], Us[:, None, :])              # d×N×M
        su, sv = self.partials(Us, Us)                                         # d×M at (u*, u*)
        live = (~self.disc)[:, None] / self.lamp[:, None]
        dmu = live * self.a2 * np.einsum("i,dij->dj", self.a, Fv)
        dvar = live * self.a2 * ((su + sv) - 2.0 * np.einsum("ij,dij->dj", W, Fv))
        if mean_grad is not None:
            dmu = dmu + np.asarray(mean_grad, float)
        return dmu, dvar
