"""Shared by tests/test_mean_program_host.py and tests/test_gpu_mean_program.py: the fixed mean closures M1–M6 (and three more for the
device shapes), the hand-built program at the size limits, seeded points, and the launch rule of the mean kernel."""
import numpy as np


def _m1(x, th):                                                   # affine, one row of coefficients per output
    return [th[0] + (th[1:7] * x).sum(), th[7] + (th[8:14] * x).sum()]


def _m2(x, th):                                                   # the example problem's shape
    return [th[0] * np.exp(x[0] / 10) * np.cos(2 * x[0]), (x[0] ** 2 - th[1]) / 64]


def _m3(x, th):                                                   # a sub-expression shared by two outputs, one constant output
    u = np.sin(x[0] * th[0]) + x[1]
    return [u * th[1], u * u + np.tanh(u), 1.5]


def _m4(x, th):                                                   # kinks
    return [np.minimum(x[0] * th[0], x[1]) + abs(x[0] - th[1]), np.maximum(th[0], x[1]) * np.abs(x[1] + 0.3)]


def _m5(x):                                                       # no parameters
    return [np.sin(x[0]) + x[1] * x[2], np.exp(-x[0] ** 2) + 0.1 * x[2]]


def _s16(x, th):                                                  # 16 outputs
    return [np.sin(x[p % 6] * th[p % 5]) + 0.1 * p * x[(p + 1) % 6] for p in range(16)]


def _t1(x, th):                                                   # three instructions: the four-wave workgroup
    return [th[0] * x[0] + np.sin(x[0])]


def _w3(x, th):                                                   # 11 inputs, 8 instructions: the three-wave workgroup with the sweep
    return [np.sin(x[0] * th[0]) + np.sin(x[1] * th[1]) + np.sin(x[2] * th[2])]


# name -> (closure, x_dim, theta_dim, y_dim)
M = {
    "M1": (_m1, 6, 14, 2),
    "M2": (_m2, 1, 2, 2),
    "M3": (_m3, 2, 2, 3),
    "M4": (_m4, 2, 2, 2),
    "M5": (_m5, 3, 0, 2),
    "S16": (_s16, 6, 5, 16),
    "T1": (_t1, 1, 1, 1),
    "W3": (_w3, 6, 5, 1),
}


def big_mean_program(api):
    """M6, the size limits by hand: d = 16, T = 16 (32 inputs, all read), output 0 with 32 constants (all read) and 64 instructions,
    output 1 a two-instruction program.  u_p = c_p y_p + y_{16+p}, w_p = c_{16+p} u_p (p < 16), q_p = w_{2p} w_{2p+1} (p < 8),
    r = the pairwise sum of the q_p, m_0 = tanh(r): no LOG, SQRT, DIV, no kink."""
    op = api.FIT_OP
    consts = list(np.linspace(0.2, 0.5, 16)) + list(np.linspace(-0.9, 0.9, 16))
    y, c, v = (lambda p: p), (lambda k: 32 + k), (lambda i: 64 + i)
    code = [(op["MUL"], y(p), c(p)) for p in range(16)]                                   # v0..15
    code += [(op["ADD"], v(p), y(16 + p)) for p in range(16)]                             # v16..31: u_p
    code += [(op["MUL"], v(16 + p), c(16 + p)) for p in range(16)]                        # v32..47: w_p
    code += [(op["MUL"], v(32 + 2 * p), v(33 + 2 * p)) for p in range(8)]                 # v48..55: q_p
    code += [(op["ADD"], v(48 + 2 * p), v(49 + 2 * p)) for p in range(4)]                 # v56..59
    code += [(op["ADD"], v(56), v(57)), (op["ADD"], v(58), v(59)), (op["ADD"], v(60), v(61)), (op["TANH"], v(62), -1)]   # v60..63
    assert len(code) == 64 and len(consts) == 32
    small = ([0.25], [(op["MUL"], 0, 31), (op["ADD"], 33, 32)], 34)                       # y_0 y_31 + 0.25 (ids: 32 = the constant, 33, 34)
    return api.MeanProgram(16, 16, [(consts, code, v(63)), small])


class HandMean:
    """A hand-built program with the face of a DeviceMean: dims, program, and the host path's callable (the numpy interpreter)."""

    def __init__(self, program):
        self.program, self.x_dim, self.theta_dim, self.y_dim = program, program.d, program.T, program.P

    def __call__(self, x, theta=None):
        return self.program.eval(np.asarray(x, float), None if theta is None else np.asarray(theta, float))[0, :, 0]


def points(seed, d, T, n, S):
    """X d×n and thetas T×S (None at T = 0), standard normal."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((d, n))
    return X, (rng.standard_normal((T, S)) if T else None)


def mean_slots(n_in, nI, grad):
    """LDS doubles per thread: y | v, twice that with the reverse sweep."""
    return (2 if grad else 1) * (n_in + nI)


def mean_waves(n_in, nI, grad, n):
    """Waves per workgroup of the mean kernel: as many of 4 as fit 64 KiB at 512 bytes per slot and wave, no more than the points
    need, at least one."""
    return max(1, min(4, 65536 // (512 * max(1, mean_slots(n_in, nI, grad))), (n + 63) // 64))
