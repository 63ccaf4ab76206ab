"""DeviceMean — the (x, θ) -> length-P closure of a Semiparametric model (src/models/semiparametric.jl:79-92,
src/models/parametric.jl:31-34,186-207), or a plain mean function x -> length-P vector (theta_dim = 0,
src/models/gaussian_process.jl:101-103), traced once into P straight-line programs over the shared inputs (api.MeanProgram,
boss_mean_t).  The mean is then evaluated on the device for all points, all outputs and all θ sets in ONE call (boss_mean_eval), which
also returns the exact ∂m/∂θ (the likelihood gradient of HipGradientMAP) and ∂m/∂x (the acquisition gradient of HipGradientAM) from
the reverse sweep — instead of one Python call per point and output, and 2T more per point for a central-difference Jacobian.

The closure is called ONCE on symbolic inputs, with the rules of DeviceFitness (fitness.py: arithmetic, the listed numpy functions,
indexing, slicing, sum, dot; no data-dependent control flow, math.*, float()).  It returns its P outputs as a list, a tuple, a traced
vector or a numpy object array; constant entries are allowed.  Limits: x_dim + theta_dim <= 32 inputs, per output 32 constants and
64 instructions, 1 <= P <= 16.  The traced programs are checked against the closure at 8 random (x, θ) points.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from . import api
from .fitness import _Sym, _SymVec, _Tracer

_LABEL = "DeviceMean"


def _extract(tr: _Tracer, out: _Sym, p: int):
    """(consts, code, out_id) of ONE output from the shared trace: the instructions and constants it reaches, renumbered in their
    original order (the outputs share sub-expressions in the trace, each program is self-contained)."""
    need_i, need_c, stack = set(), set(), [out.ref]
    while stack:
        kind, k = stack.pop()
        if kind == "c":
            need_c.add(k)
        elif kind == "i" and k not in need_i:
            need_i.add(k)
            _, a, b = tr.code[k]
            stack.append(a)
            if b is not None:
                stack.append(b)
    ci = {k: n for n, k in enumerate(sorted(need_c))}
    ii = {k: n for n, k in enumerate(sorted(need_i))}
    if len(ci) > api.MEAN_MAX_CONSTS:
        raise ValueError(f"{_LABEL}: output {p} needs {len(ci)} constants, a mean program holds at most {api.MEAN_MAX_CONSTS} per output")
    if len(ii) > api.MEAN_MAX_INSTR:
        raise ValueError(f"{_LABEL}: output {p} traces into {len(ii)} instructions, a mean program holds at most {api.MEAN_MAX_INSTR} "
                         "per output")

    def vid(ref):
        kind, k = ref
        return k if kind == "y" else tr.P + ci[k] if kind == "c" else tr.P + len(ci) + ii[k]
    code = [(api.FIT_OP[tr.code[k][0]], vid(tr.code[k][1]), -1 if tr.code[k][2] is None else vid(tr.code[k][2])) for k in sorted(need_i)]
    return [tr.consts[k] for k in sorted(need_c)], np.asarray(code, dtype=np.intc).reshape(-1, 3), vid(out.ref)


def trace_mean(closure: Callable, x_dim: int, theta_dim: int, y_dim: int) -> api.MeanProgram:
    """Trace `closure` on x_dim + theta_dim symbolic inputs and check the programs against it.  ValueError names what failed."""
    d, T, P = int(x_dim), int(theta_dim), int(y_dim)
    if d < 1 or T < 0 or d + T > api.MEAN_MAX_INPUTS:
        raise ValueError(f"{_LABEL}: x_dim = {d}, theta_dim = {T}: a mean program takes x_dim >= 1, theta_dim >= 0 and at most "
                         f"{api.MEAN_MAX_INPUTS} inputs together")
    if P < 1 or P > api.MEAN_MAX_OUTPUTS:
        raise ValueError(f"{_LABEL}: y_dim = {P}, a mean program has 1 to {api.MEAN_MAX_OUTPUTS} outputs")
    tr = _Tracer(d + T, _LABEL, "mean")
    xs = _SymVec([_Sym(tr, ("y", k)) for k in range(d)])
    out = closure(xs, _SymVec([_Sym(tr, ("y", d + t)) for t in range(T)])) if T else closure(xs)
    if isinstance(out, _Sym) and P == 1:
        out = [out]
    if isinstance(out, np.ndarray):
        out = list(out.reshape(-1)) if out.ndim else [out.item()]
    if not isinstance(out, (list, tuple, _SymVec)):
        raise ValueError(f"{_LABEL}: the closure must return its {P} outputs as a list, a tuple or a vector, it returned {type(out).__name__}")
    out = list(out)
    if len(out) != P:
        raise ValueError(f"{_LABEL}: the closure returned {len(out)} outputs, y_dim is {P}")
    outs = []
    for p, o in enumerate(out):
        if not isinstance(o, _Sym):
            try:
                o = tr.sym(o)                                # an output that ignores its inputs: a constant program
            except ValueError:
                raise ValueError(f"{_LABEL}: output {p} must be a scalar, it is {type(o).__name__}") from None
        outs.append(_extract(tr, o, p))
    prog = api.MeanProgram(d, T, outs)
    rng = np.random.default_rng(0)
    X, Th = rng.standard_normal((d, 8)), rng.standard_normal((T, 8))
    with np.errstate(all="ignore"):
        want = np.array([np.asarray(closure(X[:, k].copy(), Th[:, k].copy()) if T else closure(X[:, k].copy()), float).reshape(-1)
                         for k in range(8)])                 # 8×P
        got = np.array([prog.eval(X[:, k], Th[:, k] if T else None)[0, :, 0] for k in range(8)])
    ok = (np.isnan(want) & np.isnan(got)) | (np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))) | (got == want)
    if not np.all(ok):
        k, p = (int(i[0]) for i in np.nonzero(~ok))
        raise ValueError(f"{_LABEL}: the traced program disagrees with the closure at a test point (output {p}: closure {want[k, p]!r}, "
                         f"program {got[k, p]!r}): the closure does something the trace did not see")
    return prog


class DeviceMean:
    """The mean closure with its traced programs.  HipGaussianProcess(parametric=DeviceMean(f, d, T, P), theta_priors=...) is the
    Semiparametric model whose mean, ∂m/∂θ and ∂m/∂x come from the device; HipGaussianProcess(mean=DeviceMean(f, d, 0, P)) a plain
    prior mean function.  Calling it calls the original closure, so every host path keeps working.  `program` is the api.MeanProgram."""

    def __init__(self, closure: Callable, x_dim: int, theta_dim: int, y_dim: int):
        self.closure = closure
        self.x_dim, self.theta_dim, self.y_dim = int(x_dim), int(theta_dim), int(y_dim)
        self.program = trace_mean(closure, x_dim, theta_dim, y_dim)

    def __call__(self, x, theta=None):
        return self.closure(x, theta) if self.theta_dim else self.closure(x)

    def evaluate(self, X, thetas=None, layout: int = api.MEAN_SAMPLE_MAJOR, jac_theta: bool = False, jac_x: bool = False, device: int = 0):
        """(m, ∂m/∂θ or None, ∂m/∂x or None) at the columns of X for every column of thetas in one device call
        (api.MeanProgram.eval_device)."""
        return self.program.eval_device(X, thetas, layout, jac_theta, jac_x, device)


def device_mean_of(model) -> Optional[DeviceMean]:
    """The DeviceMean behind a model's prior mean, or None (a plain closure, a constant, no mean)."""
    for f in (getattr(model, "parametric", None), getattr(model, "mean", None)):
        if isinstance(f, DeviceMean):
            return f
    return None
