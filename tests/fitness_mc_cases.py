"""Shared by tests/test_fitness_program_host.py and tests/test_gpu_fitness_mc.py: the six fixed fitness closures, seeded moments, and
the numpy reference of the Monte-Carlo acquisition gradient (the formula of the header, from FitnessProgram.grad)."""
import math

import numpy as np
from scipy.special import erfc

_W16 = np.linspace(0.5, 2.0, 16) / 16.0

# name -> (closure, y_dim)
F = {
    "F1": (lambda y: np.cos(y[0]) + np.sin(y[1]), 2),
    "F2": (lambda y: -(y[0] - 0.3) ** 2 - 0.5 * (y[1] + 0.1) ** 2, 2),
    "F3": (lambda y: np.minimum(y[0], y[1]) - 0.1 * np.abs(y[2]), 3),
    "F4": (lambda y: np.tanh(y[0]) * np.exp(-0.5 * y[1]) + np.log(1 + y[0] ** 2) + np.sqrt(1 + y[1] ** 2) / (2 + np.cos(y[0]))
           + np.maximum(y[0], -y[1]) * (1 + y[0] ** 2) ** 0.75, 2),
    "F5": (lambda y: (_W16 * y ** 2).sum(), 16),
    "F6": (lambda y: 0.7 * y[0] - 0.2 * y[1], 2),
    "G1": (lambda y: np.sin(y[0]) - 0.1 * y[0] ** 2, 1),          # a one-output fitness for the P = 1 shapes
}


def moments(seed, S, P, M, d=None):
    """mu in [-1, 1], var in [0, 1] ([S][P][M]); with d also dmu, dvar in [-1, 1] ([S][P][d][M])."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-1, 1, (S, P, M))
    var = rng.uniform(0, 1, (S, P, M))
    if d is None:
        return mu, var
    return mu, var, rng.uniform(-1, 1, (S, P, d, M)), rng.uniform(-1, 1, (S, P, d, M))


def eps_for(seed, S, P, K):
    """P×K at S = 1, P×S otherwise (sample s takes column s)."""
    return np.random.default_rng(seed).standard_normal((P, K if S == 1 else S))


def clip(var):
    return np.where((var < 0) & (var >= -1e-8), 0.0, var)


def f_values(prog, mu, var, eps):
    """f at every (sample, candidate, ε): list over s of M×K arrays (S = 1: all columns; S > 1: column s)."""
    S, P, M = mu.shape
    out = []
    for s in range(S):
        e = eps if S == 1 else eps[:, s:s + 1]
        Y = mu[s][:, :, None] + np.sqrt(np.maximum(var[s], 0.0))[:, :, None] * e[:, None, :]
        out.append(prog.eval(Y.reshape(P, -1)).reshape(M, -1))
    return out


def _cdf(z):
    return 0.5 * erfc(-np.asarray(z, float) / math.sqrt(2.0))


def _pdf(z):
    return np.exp(-0.5 * np.asarray(z, float) ** 2) / math.sqrt(2.0 * math.pi)


def ref_value_and_grad(prog, mu, var, dmu, dvar, eps, y_max, best, mask):
    """(acq[M], dacq[d, M]) by the formula: per sample EI = mean_k max(0, f_k - best), grad EI = (1/K) sum_p (A_p grad mu_p + B_p grad sd_p),
    A_p = sum_k 1[f_k > best] df/dy_p, B_p = sum_k 1[f_k > best] df/dy_p eps_pk, grad sd_p = grad var_p / (2 sd_p) (0 where the variance
    is clipped or 0); acq = EI FP, grad acq = grad EI FP + EI grad FP; poisoned in any sample: -Inf and 0; masked: 0 and 0; mean over s."""
    S, P, M = mu.shape
    d = dmu.shape[2]
    acq, dacq = np.zeros(M), np.zeros((d, M))
    if best is None and y_max is None:                            # construct_ei(…, nothing, …, nothing): 0 before anything is looked at
        return acq, dacq
    for s in range(S):
        e = eps if S == 1 else eps[:, s:s + 1]
        K = e.shape[1]
        v = np.where(var[s] < 0, 0.0, var[s])
        poison = np.any(var[s] < -1e-8, axis=0)
        sd = np.sqrt(v)
        pos = var[s] > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            dsd = np.where(pos[:, None, :], dvar[s] / (2.0 * sd[:, None, :]), 0.0)
        ei, dei = np.zeros(M), np.zeros((d, M))
        if best is not None:
            Y = mu[s][:, :, None] + sd[:, :, None] * e[:, None, :]
            f = prog.eval(Y.reshape(P, -1)).reshape(M, K)
            G = prog.grad(Y.reshape(P, -1)).reshape(P, M, K)
            ind = f > best
            ei = np.where(ind, f - best, 0.0).sum(1) / K
            A = (G * ind[None]).sum(2)
            B = (G * ind[None] * e[:, None, :]).sum(2)
            dei = ((A[:, None, :] * dmu[s]).sum(0) + (B[:, None, :] * dsd).sum(0)) / K
        fp, dfp = np.ones(M), np.zeros((d, M))
        if y_max is not None:
            ym = np.asarray(y_max, float)
            phis = np.ones((P, M))
            for p in range(P):
                if np.isinf(ym[p]) and ym[p] > 0:
                    continue
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = (ym[p] - mu[s, p]) / sd[p]
                t = np.where((sd[p] == 0) & (ym[p] == mu[s, p]), np.inf, t)
                phis[p] = _cdf(t)
            fp = phis.prod(0)
            for p in range(P):
                if np.isinf(ym[p]) and ym[p] > 0:
                    continue
                others = np.prod(np.delete(phis, p, axis=0), axis=0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = (ym[p] - mu[s, p]) / sd[p]
                    dt = -dmu[s, p] / sd[p] - (ym[p] - mu[s, p]) * dvar[s, p] / (2.0 * sd[p] * v[p])
                    term = others * _pdf(t) * dt
                dfp += np.where(pos[p][None, :], term, 0.0)
        if best is None:
            a, g = (fp, dfp) if y_max is not None else (np.zeros(M), np.zeros((d, M)))
        else:
            a, g = ei * fp, dei * fp + ei * dfp
        acq += np.where(poison, -np.inf, a)
        dacq += np.where(poison[None, :], 0.0, g)
    acq, dacq = acq / S, np.where(np.isneginf(acq)[None, :], 0.0, dacq / S)     # -Inf in any sample: gradient 0
    if mask is not None:
        m = np.asarray(mask, bool)
        acq, dacq = np.where(m, acq, 0.0), np.where(m[None, :], dacq, 0.0)
    return acq, dacq
