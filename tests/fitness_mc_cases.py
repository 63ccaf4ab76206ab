"""Shared by tests/test_fitness_program_host.py and tests/test_gpu_fitness_mc.py: the fixed fitness closures, the hand-built program at
the size limits, the launch rule of the two Monte-Carlo kernels, seeded moments, the numpy reference of the Monte-Carlo acquisition
gradient (the formula of the header, from FitnessProgram.grad) and a 50-digit interpreter of a program (forward values only) whose
central differences pin the derivative without any differentiation rule."""
import math

import numpy as np
from scipy.special import erfc

_W16 = np.linspace(0.5, 2.0, 16) / 16.0


def _wsin(n):
    """sum_p w_p sin(y_p + o_p) on n inputs: 3n + (n - 1) instructions, smooth everywhere."""
    off, w = np.linspace(0.1, 0.8, n), np.linspace(0.5, 1.5, n) / n
    return lambda y: (np.sin(y + off) * w).sum()


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
    # sized for the workgroup shapes no closure above reaches (mc_waves; asserted by the tests from the traced P and instruction count)
    "W3g": (lambda y: np.sin(y[0]) * np.cos(y[1]) + np.tanh(y[2]) * y[0] - 0.25 * y[1] ** 2, 3),      # gradient kernel: 3 waves
    "W3v": (_wsin(6), 6),                                         # value kernel: 3 waves
    "W2v": (_wsin(8), 8),                                         # value kernel: 2 waves
}


def mc_slots(P, nI, grad):
    """LDS doubles per thread: mu | sd | y | v (value kernel), twice that for the reverse sweep and the sums (gradient kernel)."""
    return 6 * P + 2 * nI if grad else 3 * P + nI


def mc_waves(P, nI, grad):
    """Waves per workgroup of a Monte-Carlo kernel: as many of 4 as fit 64 KiB at 512 bytes per slot and wave, at least one."""
    return max(1, min(4, 65536 // (512 * mc_slots(P, nI, grad))))


def big_program(api):
    """The size limits by hand: P = 16 inputs, 32 constants, 64 instructions; every input and constant is read, and r (v54) feeds
    four later instructions.  u_p = a_p y_p + b_p (|u| <= 2.9 on |y| <= 5), r = sum_{p<8} sin(u_p) u_{8+p},
    f = 0.5 (r² + r tanh r + exp(tanh r) - cos r): no LOG, SQRT, DIV, no kink."""
    op = api.FIT_OP
    consts = list(np.linspace(0.2, 0.5, 16)) + list(np.linspace(-0.4, 0.4, 16))
    y, c, v = (lambda p: p), (lambda k: 16 + k), (lambda i: 48 + i)
    code = [(op["MUL"], y(p), c(p)) for p in range(16)]                                   # v0..15
    code += [(op["ADD"], v(p), c(16 + p)) for p in range(16)]                             # v16..31: u_p
    code += [(op["SIN"], v(16 + p), -1) for p in range(8)]                                # v32..39
    code += [(op["MUL"], v(32 + p), v(24 + p)) for p in range(8)]                         # v40..47
    code += [(op["ADD"], v(40), v(41))] + [(op["ADD"], v(47 + p), v(41 + p)) for p in range(1, 7)]   # v48..54: r = v54
    r = v(54)
    code += [(op["TANH"], r, -1), (op["SQUARE"], r, -1), (op["MUL"], r, v(55)), (op["ADD"], v(56), v(57)),      # v55..58
             (op["EXP"], v(55), -1), (op["ADD"], v(58), v(59)), (op["COS"], r, -1), (op["SUB"], v(60), v(61)),  # v59..62
             (op["MUL"], v(62), c(15))]                                                                         # v63
    assert len(code) == 64 and len(consts) == 32
    return api.FitnessProgram(16, consts, code, v(63))


class HandFitness:
    """A hand-built program with the face of a DeviceFitness: y_dim, program, and the host path's callable (the numpy interpreter)."""

    def __init__(self, program):
        self.program, self.y_dim = program, program.P

    def __call__(self, y):
        return self.program.eval(np.asarray(y, float))


# ------------------------------------------------------------------------------------------ 50-digit interpreter
_OPS = ("ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQUARE", "SQRT", "EXP", "LOG", "SIN", "COS", "TANH", "POW", "MIN", "MAX")


def mp_eval(prog, y):
    """(f, distance to the nearest kink) of prog at the point y (P mpmath numbers), forward values only, in the current mpmath
    precision.  MIN / MAX give NaN when either operand is NaN.  The kink distance is min |x| over ABS and min |x - z| over MIN / MAX."""
    import mpmath as mp
    vals = [mp.mpf(t) for t in y] + [mp.mpf(float(c)) for c in prog.consts]
    kink = mp.inf
    for o, a, b in prog.code:
        x, z, name = vals[a], (vals[b] if b >= 0 else None), _OPS[o]
        if name == "ADD": r = x + z
        elif name == "SUB": r = x - z
        elif name == "MUL": r = x * z
        elif name == "DIV": r = x / z
        elif name == "NEG": r = -x
        elif name == "ABS": r, kink = abs(x), min(kink, abs(x))
        elif name == "SQUARE": r = x * x
        elif name == "SQRT": r = mp.sqrt(x)
        elif name == "EXP": r = mp.exp(x)
        elif name == "LOG": r = mp.log(x)
        elif name == "SIN": r = mp.sin(x)
        elif name == "COS": r = mp.cos(x)
        elif name == "TANH": r = mp.tanh(x)
        elif name == "POW": r = mp.power(x, z)
        elif mp.isnan(x) or mp.isnan(z): r = mp.nan
        else:
            r = (x if x <= z else z) if name == "MIN" else (x if x >= z else z)
            kink = min(kink, abs(x - z))
        vals.append(r)
    return vals[prog.out_id], kink


def mp_grad(prog, Y, h="1e-20", dps=50):
    """(df/dy [P, n] as float64, min kink distance) at the columns of Y by central differences in dps-digit arithmetic: truncation
    about h² |f³| ~ 1e-40, rounding about 10^-dps / h = 1e-30 — no differentiation rule enters."""
    import mpmath as mp
    Y = np.asarray(Y, float).reshape(prog.P, -1)
    g = np.zeros(Y.shape)
    kink = math.inf
    with mp.workdps(dps):
        hh = mp.mpf(h)
        for k in range(Y.shape[1]):
            y0 = [mp.mpf(float(t)) for t in Y[:, k]]
            kink = min(kink, float(mp_eval(prog, y0)[1]))
            for p in range(prog.P):
                yp, ym = list(y0), list(y0)
                yp[p], ym[p] = y0[p] + hh, y0[p] - hh
                g[p, k] = float((mp_eval(prog, yp)[0] - mp_eval(prog, ym)[0]) / (2 * hh))
    return g, kink


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
