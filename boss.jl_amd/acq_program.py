"""DeviceAcquisition — a user-defined acquisition function ("Defining custom acquisition function", src/types/acquisition.jl:1-57)
whose closure over the posterior moments of one candidate has been traced into a straight-line program (api.AcqProgram,
boss_acqp_t).  The device evaluates it behind the prediction (boss_acq_prog*), with the conventions of the built-in EI: the average
over the BI samples, the domain mask (construct_safe_acquisition, src/acquisition.jl:21-25), the negative-variance rule, the
first-index arg-max and the gradient w.r.t. the candidate.

The closure is `closure(mu, var, q) -> scalar`: mu and var are the P posterior means and variances of one candidate under one
hyper-parameter sample, q the Q runtime scalars `params(problem)` returns once per maximize_acquisition call (best-so-far, β_t, y_max:
what changes every BO iteration and must not be a traced constant).  It is called ONCE on symbolic inputs, under the rules of
DeviceFitness (fitness.py); beyond those, normcdf / normpdf of this module and scipy.special.ndtr are traced into the program's
NORMCDF / NORMPDF opcodes.  The traced program is then checked against the closure at 8 seeded points with positive variances.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
from scipy import special as _sp

from . import api
from .fitness import _Sym, _SymVec, _Tracer, _tracer_of
from .problem import LinFitness, best_so_far


class _AcqTracer(_Tracer):
    extra_ufuncs = {_sp.ndtr: "NORMCDF"}                     # (fitness._apply_ufunc asks the tracer for these)
    acq_ops = True

    def __init__(self, P: int, Q: int):
        super().__init__(2 * P + Q, "DeviceAcquisition", "acquisition")
        self.y_dim, self.n_params = P, Q

    def program(self, out: _Sym) -> api.AcqProgram:
        nc = len(self.consts)
        if nc > api.FIT_MAX_CONSTS:
            raise ValueError(f"{self.label}: the closure needs {nc} constants, an acquisition program holds at most {api.FIT_MAX_CONSTS}")
        if len(self.code) > api.FIT_MAX_INSTR:
            raise ValueError(f"{self.label}: the closure traces into {len(self.code)} instructions, an acquisition program holds at most "
                             f"{api.FIT_MAX_INSTR}")

        def vid(ref):
            kind, k = ref
            return k if kind == "y" else self.P + k if kind == "c" else self.P + nc + k
        code = [(api.ACQ_OP[op], vid(a), -1 if b is None else vid(b)) for op, a, b in self.code]
        return api.AcqProgram(self.y_dim, self.n_params, self.consts, np.asarray(code, dtype=np.intc).reshape(-1, 3), vid(out.ref))


def _normal(op: str, numeric: Callable, z):
    if isinstance(z, (_Sym, _SymVec)):
        tr = _tracer_of(z)
        if not getattr(tr, "acq_ops", False):
            raise ValueError(f"{tr.label}: {op.lower()} is not supported in a device {tr.noun}")
        if isinstance(z, _SymVec):
            return _SymVec([tr.emit(op, it) for it in z.items])
        return tr.emit(op, z)
    return numeric(np.asarray(z, dtype=np.float64)) if not np.isscalar(z) else float(numeric(np.float64(z)))


def normcdf(z):
    """Φ(z) = erfc(−z/√2)/2: on a traced value the NORMCDF opcode (in a DeviceAcquisition closure only), on numbers and arrays the
    same formula."""
    return _normal("NORMCDF", api._normcdf, z)


def normpdf(z):
    """φ(z) = exp(−z²/2)/√(2π): on a traced value the NORMPDF opcode (in a DeviceAcquisition closure only), on numbers and arrays the
    same formula."""
    return _normal("NORMPDF", api._normpdf, z)


def trace_acquisition(closure: Callable, y_dim: int, n_params: int = 0) -> api.AcqProgram:
    """Trace `closure(mu, var, q)` on symbolic inputs and check the program against the closure.  ValueError names what failed."""
    P, Q = int(y_dim), int(n_params)
    if P < 1 or P > api.ACQ_MAX_OUTPUTS:
        raise ValueError(f"DeviceAcquisition: y_dim = {P}, an acquisition program takes the moments of 1 to {api.ACQ_MAX_OUTPUTS} outputs")
    if Q < 0 or Q > api.ACQ_MAX_SCALARS:
        raise ValueError(f"DeviceAcquisition: n_params = {Q}, an acquisition program takes 0 to {api.ACQ_MAX_SCALARS} runtime scalars")
    tr = _AcqTracer(P, Q)
    ins = [_Sym(tr, ("y", k)) for k in range(2 * P + Q)]
    out = closure(_SymVec(ins[:P]), _SymVec(ins[P:2 * P]), _SymVec(ins[2 * P:]))
    if isinstance(out, _SymVec) and len(out) == 1:
        out = out[0]
    if isinstance(out, np.ndarray) and out.size == 1:
        out = out.reshape(-1)[0]
    if not isinstance(out, _Sym):
        try:
            out = tr.sym(out)                                # a closure that ignores its inputs: a constant program
        except ValueError:
            raise ValueError(f"DeviceAcquisition: the closure must return one scalar, it returned {type(out).__name__}") from None
    prog = tr.program(out)
    rng = np.random.default_rng(0)
    mu, var, q = rng.standard_normal((P, 8)), rng.uniform(0.05, 2.0, (P, 8)), rng.standard_normal((Q, 8))
    with np.errstate(all="ignore"):
        want = np.array([float(closure(mu[:, k].copy(), var[:, k].copy(), q[:, k].copy())) for k in range(8)])
    got = prog.eval(np.vstack([mu, var, q]))
    ok = (np.isnan(want) & np.isnan(got)) | (np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))) | (got == want)
    if not np.all(ok):
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"DeviceAcquisition: the traced program disagrees with the closure at a test point (closure {want[k]!r}, program "
                         f"{got[k]!r}): the closure does something the trace did not see")
    return prog


class DeviceAcquisition:
    """AcquisitionFunction whose construct_acquisition runs on the device.
      closure    (mu, var, q) -> scalar, traced once (module docstring);
      y_dim      P, the number of outputs (1..8);
      n_params   Q, the number of runtime scalars (0..16);
      params     problem -> Q floats, called once per maximize_acquisition (non-finite values are allowed: y_max = +Inf);
      cons_safe  mask candidates outside the bounds and constraints, as ExpectedImprovement does;
      outside    the value of a masked candidate (-Inf: construct_safe_acquisition; not 0 — a custom acquisition may be negative
                 everywhere).
    `fitness` (optional attribute): what get_fitness would return, for callers that ask the acquisition for it."""

    fitness = None

    def __init__(self, closure: Callable, y_dim: int, n_params: int = 0, params: Optional[Callable] = None, cons_safe: bool = True,
                 outside: float = -np.inf):
        self.closure = closure
        self.y_dim, self.n_params = int(y_dim), int(n_params)
        if self.n_params > 0 and params is None:
            raise ValueError(f"DeviceAcquisition: n_params = {self.n_params} needs params(problem) -> {self.n_params} floats")
        self.params = params
        self.cons_safe = bool(cons_safe)
        self.outside = float(outside)
        self.program = trace_acquisition(closure, self.y_dim, self.n_params)

    def __call__(self, mu, var, q=None):
        """The closure itself on numbers (the host path: one candidate, one sample)."""
        q = np.zeros(0) if q is None else np.asarray(q, float)
        return float(self.closure(np.asarray(mu, float), np.asarray(var, float), q))

    def scalars(self, problem) -> np.ndarray:
        """q of this maximisation: params(problem), checked for its length."""
        if problem.data.Y.shape[0] != self.y_dim:
            raise ValueError(f"DeviceAcquisition: traced for y_dim = {self.y_dim}, the problem has {problem.data.Y.shape[0]} outputs")
        if self.n_params == 0:
            return np.zeros(0)
        q = np.asarray(self.params(problem), dtype=np.float64).reshape(-1)
        if q.shape[0] != self.n_params:
            raise ValueError(f"DeviceAcquisition: params(problem) returned {q.shape[0]} values, n_params = {self.n_params}")
        return q


class UpperConfidenceBound(DeviceAcquisition):
    """cᵀμ + β·sqrt((c²)ᵀσ²) for a LinFitness c (GP-UCB).  β is a traced constant."""

    def __init__(self, fitness: LinFitness, beta: float, cons_safe: bool = True, outside: float = -np.inf):
        c = np.asarray(fitness.coefs, dtype=np.float64).reshape(-1)
        beta = float(beta)
        super().__init__(lambda mu, var, q: mu @ c + beta * np.sqrt(var @ (c * c)), c.shape[0], cons_safe=cons_safe, outside=outside)
        self.fitness, self.beta = fitness, beta


class ProbabilityOfImprovement(DeviceAcquisition):
    """Φ((cᵀμ − best − ξ)/σ_f) · Π_p Φ((y_max_p − μ_p)/σ_p) for a LinFitness c, σ_f = sqrt((c²)ᵀσ²).  best and y_max are runtime
    scalars (q = [best, y_max_1..P]); with nothing feasible seen yet best = −Inf and the value is the feasibility alone, as the
    reference's EI gives."""

    def __init__(self, fitness: LinFitness, xi: float = 0.0, cons_safe: bool = True, outside: float = -np.inf):
        c = np.asarray(fitness.coefs, dtype=np.float64).reshape(-1)
        P, xi = c.shape[0], float(xi)

        def closure(mu, var, q):
            a = normcdf((mu @ c - q[0] - xi) / np.sqrt(var @ (c * c)))
            for p in range(P):
                a = a * normcdf((q[1 + p] - mu[p]) / np.sqrt(var[p]))
            return a

        def params(problem):
            b = best_so_far(fitness, problem.data.Y, problem.y_max)
            return np.concatenate([[-np.inf if b is None else b], np.asarray(problem.y_max, float)])
        super().__init__(closure, P, n_params=1 + P, params=params, cons_safe=cons_safe, outside=outside)
        self.fitness, self.xi = fitness, xi
