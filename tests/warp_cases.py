"""What tests/golden/make_warp.py, tests/test_warp_host.py and tests/test_gpu_warp.py share: the transform cases, the fixture, the bars
and the launch rule restated.

Transforms are written once over a function namespace F (numpy for tracing and the device, mpmath for the 50-digit truths):
    feature   x -> (x0, x0·x1, sin x1)                                              d_user 2 -> d_model 3
    kuma      x -> (1 − (1 − (x0/1.5)^1.5)^0.8, log(x1 + x2 + 0.5))                 3 -> 2   (Kumaraswamy cdf, log)
    logw      x -> (log(x0 + 0.1), log(x1 + 0.5·x0 + 0.1))                          2 -> 2   (coupled: J is not symmetric)
    log       (y_, s_) -> (log y_, s_/y_)                   P = 1, joint            (the docstring example of transformed.jl:38-43)
    mix       (y_, s_) -> (0.8y0 + 0.3y1, y1 − 0.5y0), s = sqrt of the mixed squares   P = 2, joint
    affine    y_i -> a_i y_i + b_i, s_i -> a_i s_i, a = (2, −2)   P = 2, sliced: a negative a gives a NEGATIVE std, var = std² all the same
Every Jacobian entry of these lies in [1e-3, 1e3] on the fixture's points (asserted by the generator).

Fixture (tests/golden/warp.json): per case the model-space training data, hyper-parameters, cond(K) per output, user-space candidates
and the 50-digit truths rounded to fp64 — X_, J, the model-space moments and gradients at the exact warped points, the user-space
(mu, var, dmu, dvar) of the whole chain, and "fold_*": the moments stage applied, at 50 digits, to the ROUNDED model-space arrays
(what boss_warp_moments_host is given).

Bars of the chain (first-order error propagation, no new constant): with the regimes bars of output q (regimes_cases.py:
8B(1 + max|mu_|), 8B·amp², 100B(1 + max|grad|), B = cond·N·u),
    L = max(1, max |∂(mu, var)/∂(mu_, var_)| at the truth),   Jm = max(1, max|J|)
    values:     L · sum_q (bar(mu_q) + bar(var_q))            |Δout| <= sum_in |∂out/∂in| |Δin|
    gradients:  L · Jm · sum_q (bar(dmu_q) + bar(dvar_q))
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "warp.json")
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------ transforms over a namespace F
def feature(x, F):
    return [x[0], x[0] * x[1], F.sin(x[1])]


def kuma(x, F):
    return [1.0 - (1.0 - (x[0] / 1.5) ** 1.5) ** 0.8, F.log(x[1] + x[2] + 0.5)]


def logw(x, F):
    return [F.log(x[0] + 0.1), F.log(x[1] + 0.5 * x[0] + 0.1)]


def out_log(y, s, F):
    return [F.log(y[0])], [s[0] / y[0]]


def out_mix(y, s, F):
    return ([0.8 * y[0] + 0.3 * y[1], y[1] - 0.5 * y[0]],
            [F.sqrt((0.8 * s[0]) ** 2 + (0.3 * s[1]) ** 2), F.sqrt(s[1] ** 2 + (0.5 * s[0]) ** 2)])


AFFINE = ((2.0, 1.0), (-2.0, 0.5))


def out_affine(y, s, F):
    return [a * y[i] + b for i, (a, b) in enumerate(AFFINE)], [a * s[i] for i, (a, _) in enumerate(AFFINE)]


def back_log(y):
    return np.exp(y)


def back_mix(y):
    y0 = (y[0] - 0.3 * y[1]) / 0.95                          # inverse of [[0.8, 0.3], [-0.5, 1]]
    return np.array([y0, y[1] + 0.5 * y0])


# name -> (d_user, d_model, N, M, P, input warp, output transform, kernel, "joint" | "sliced")
CASES = {
    "feature-log": (2, 3, 12, 6, 1, feature, out_log, "matern52", "joint"),
    "kuma-mix": (3, 2, 12, 6, 2, kuma, out_mix, "sqexp", "joint"),
    "logw-affine": (2, 2, 40, 6, 2, logw, out_affine, "matern52", "sliced"),
}
PRIOR_MEAN = 2.0                                             # constant prior mean of every output (keeps mu_ > 0 under out_log)


def hyper(name):
    """lengthscale[d_model], amplitude[P], noise_std[P] of a case."""
    _, dm, _, _, P = CASES[name][:5]
    return np.full(dm, 0.6 * np.sqrt(dm)), 0.5 + 0.2 * np.arange(P), 0.05 + 0.02 * np.arange(P)


def data(name):
    """User-space X (d_user×N), candidates Xs (d_user×M) in [0.2, 1.2]^d and the model-space training set (X_ = warp(X) rounded to
    fp64, Y_ P×N) the handles are fitted on."""
    du, dm, N, M, P, win, _, _, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    X = rng.uniform(0.2, 1.2, (du, N))
    Xs = rng.uniform(0.25, 1.15, (du, M))
    X_ = np.array([np.asarray(win(X[:, j], np), float) for j in range(N)]).T
    Y_ = np.stack([PRIOR_MEAN + 0.4 * np.sin(2.0 * X_.sum(0) + p) + 0.02 * rng.standard_normal(N) for p in range(P)])
    return X, Xs, np.asfortranarray(X_), Y_


def in_closure(name):
    win = CASES[name][5]
    return lambda x: win(x, np)


def out_closure(name):
    wout = CASES[name][6]
    return lambda y, s: wout(y, s, np)


def sliced_closures(name):
    """The per-output scalar closures of a sliced case."""
    assert CASES[name][8] == "sliced"
    return ([(lambda y, s, a=a, b=b: (a * y + b, a * s)) for a, b in AFFINE], [(lambda y, a=a, b=b: (y - b) / a) for a, b in AFFINE])


def warp_program(B, name, with_in=True, with_out=True):
    """api.WarpProgram of a case from its traced closures."""
    du, dm, _, _, P = CASES[name][:5]
    ip = B.trace_mean(in_closure(name), du, 0, dm) if with_in else None
    op = None
    if with_out:
        f = out_closure(name)

        def packed(z):
            m, s = f(z[:P], z[P:])
            return list(m) + list(s)
        op = B.trace_mean(packed, 2 * P, 0, 2 * P)
    return B.api.WarpProgram(ip, P, op)


_fx = None


def load():
    global _fx
    if _fx is None:
        with open(PATH) as f:
            fx = json.load(f)
        for c in fx["cases"].values():
            for k, v in c.items():
                if isinstance(v, list):
                    c[k] = np.asarray(v, dtype=np.float64)
        _fx = fx
    return _fx


# ------------------------------------------------------------------------------------------ bars
def regimes_bars(c, N):
    """Per output q: (bar mu_, bar var_, bar dmu_, bar dvar_) by the formulas of regimes_cases.py."""
    out = []
    for q in range(c["mu_"].shape[0]):
        B = c["cond"][q] * N * U
        m8, m100 = (8 * B, 100 * B) if B >= 8 * U else (64 * U, 64 * U)
        out.append((m8 * (1 + np.abs(c["mu_"][q]).max()), m8 * (c["amp"][q] + 1e-8) ** 2, m100 * (1 + np.abs(c["dmu_"][q]).max()),
                    m100 * (1 + np.abs(c["dvar_"][q]).max())))
    return out


def chain_bars(c, N):
    """(value bar, gradient bar) of the user-space results of a case (module docstring)."""
    rb = regimes_bars(c, N)
    L, Jm = max(1.0, float(c["L"])), max(1.0, float(np.abs(c["J"]).max()))
    return L * sum(b[0] + b[1] for b in rb), L * Jm * sum(b[2] + b[3] for b in rb)


# ------------------------------------------------------------------------------------------ the launch rule, restated
def slots_x(d_user, nI, grad):
    return (2 if grad else 1) * (d_user + nI)


def slots_m(P, nI, d_model, grad):
    return (2 if grad else 1) * (2 * P + nI) + (d_model if grad else 0)


def waves(slots, n):
    """Waves per workgroup: as many of 4 as fit 64 KiB at 512 bytes per slot and wave, no more than the candidates need, at least 1."""
    per = 512 * max(1, slots)
    return max(1, min(max(1, min(4, (64 * 1024) // per)), (n + 63) // 64))


def big_program(api, n_in, n_out):
    """A hand-built mean program over n_in inputs with n_out outputs of 64 instructions each: a chain
    v0 = x_r mod n_in · c0,  v_i = sin(v_{i-1}) + x_{i mod n_in} alternating with v_i = v_{i-1} · c1."""
    outs = []
    for r in range(n_out):
        consts = [0.5 + 0.01 * r, 0.9]
        base = n_in + 2
        code = [(api.FIT_OP["MUL"], r % n_in, n_in)]
        i = 1
        while i < 64:
            prev = base + i - 1
            if i % 3 == 1:
                code.append((api.FIT_OP["SIN"], prev, -1))
            elif i % 3 == 2:
                code.append((api.FIT_OP["ADD"], prev, i % n_in))
            else:
                code.append((api.FIT_OP["MUL"], prev, n_in + 1))
            i += 1
        outs.append((consts, np.asarray(code, dtype=np.intc), base + 63))
    return api.MeanProgram(n_in, 0, outs)
