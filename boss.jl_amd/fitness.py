"""DeviceFitness — a NonlinFitness whose closure has been traced into a straight-line program (api.FitnessProgram,
boss_fit_t), so that expected_improvement(::NonlinFitness) (src/acquisitions/expected_improvement.jl:104-111) and its gradient
run on the device (boss_acq_ei_mc*) instead of calling the closure once per candidate and ε-sample on the host.

The closure is called ONCE on symbolic inputs.  What it may do with them: + - * / **, unary -, abs; np.sin, np.cos, np.exp,
np.log, np.sqrt, np.tanh, np.abs, np.square, np.power, np.minimum, np.maximum on an element or on the whole vector; indexing,
slicing, iteration, y.sum(), y @ w, np.dot.  Anything whose result depends on the VALUE of an input in another way — `if y[0] > 0`,
math.sin(y[0]), float(y[0]) — cannot be traced and raises ValueError, as does an unsupported function or a program beyond the
limits (16 inputs, 32 constants, 64 instructions).  The traced program is then checked against the closure at 8 random points.
"""
from __future__ import annotations

import numbers
from typing import Callable

import numpy as np

from . import api
from .problem import NonlinFitness

_UFUNC_OPS = {np.add: "ADD", np.subtract: "SUB", np.multiply: "MUL", np.true_divide: "DIV", np.negative: "NEG", np.absolute: "ABS",
              np.square: "SQUARE", np.sqrt: "SQRT", np.exp: "EXP", np.log: "LOG", np.sin: "SIN", np.cos: "COS", np.tanh: "TANH",
              np.power: "POW", np.minimum: "MIN", np.maximum: "MAX"}


class _Tracer:
    def __init__(self, P: int, label: str = "DeviceFitness", noun: str = "fitness"):
        self.P = P
        self.label, self.noun = label, noun   # who speaks in the error messages (DeviceMean traces with the same classes, mean.py)
        self.consts = []                 # values, in id order
        self.const_id = {}               # bit pattern -> value id
        self.code = []                   # (op, a, b)
        self.memo = {}                   # (op, a, b) -> value id: a repeated sub-expression is one instruction

    def const(self, c) -> "_Sym":
        c = float(c)
        if not np.isfinite(c):
            raise ValueError(f"{self.label}: the closure uses a constant that is not finite")
        key = np.float64(c).tobytes()
        if key not in self.const_id:
            self.const_id[key] = len(self.consts)
            self.consts.append(c)
        return _Sym(self, ("c", self.const_id[key]))

    def sym(self, x) -> "_Sym":
        if isinstance(x, _Sym):
            return x
        if isinstance(x, (numbers.Real, np.floating, np.integer)) or (isinstance(x, np.ndarray) and x.ndim == 0):
            return self.const(x)
        raise ValueError(f"{self.label}: cannot trace an operand of type {type(x).__name__}")

    def emit(self, op: str, a, b=None) -> "_Sym":
        a = self.sym(a)
        key = (op, a.ref, None if b is None else self.sym(b).ref)
        if key not in self.memo:
            self.memo[key] = len(self.code)
            self.code.append(key)
        return _Sym(self, ("i", self.memo[key]))

    def program(self, out: "_Sym") -> api.FitnessProgram:
        nc = len(self.consts)
        if nc > api.FIT_MAX_CONSTS:
            raise ValueError(f"{self.label}: the closure needs {nc} constants, a {self.noun} program holds at most {api.FIT_MAX_CONSTS}")
        if len(self.code) > api.FIT_MAX_INSTR:
            raise ValueError(f"{self.label}: the closure traces into {len(self.code)} instructions, a {self.noun} program holds at most "
                             f"{api.FIT_MAX_INSTR}")

        def vid(ref):
            kind, k = ref
            return k if kind == "y" else self.P + k if kind == "c" else self.P + nc + k
        code = [(api.FIT_OP[op], vid(a), -1 if b is None else vid(b)) for op, a, b in self.code]
        return api.FitnessProgram(self.P, self.consts, np.asarray(code, dtype=np.intc).reshape(-1, 3), vid(out.ref))


def _label_of(*xs) -> str:
    """The label of the tracer behind the first traced operand ("DeviceFitness" where there is none to ask)."""
    for x in xs:
        if isinstance(x, _Sym):
            return x.tr.label
        if isinstance(x, _SymVec) and x.items:
            return x.items[0].tr.label
    return "DeviceFitness"


def _noun_of(*xs) -> str:
    for x in xs:
        if isinstance(x, _Sym):
            return x.tr.noun
        if isinstance(x, _SymVec) and x.items:
            return x.items[0].tr.noun
    return "fitness"


def _no_value(what):
    def raiser(self, *a, **k):
        raise ValueError(f"{_label_of(self)}: the closure {what}: its result would depend on the value of an input, which a traced "
                         "program cannot express (data-dependent control flow, math.* functions and float() are not traceable; "
                         "use the numpy functions and np.minimum / np.maximum)")
    return raiser


class _Sym:
    """One traced scalar."""
    __array_priority__ = 1000.0

    def __init__(self, tr: _Tracer, ref):
        self.tr, self.ref = tr, ref

    def __add__(self, o): return _binary("ADD", self, o)
    def __radd__(self, o): return self if (isinstance(o, int) and o == 0) else _binary("ADD", o, self)   # (the 0 of builtin sum)
    def __sub__(self, o): return _binary("SUB", self, o)
    def __rsub__(self, o): return _binary("SUB", o, self)
    def __mul__(self, o): return _binary("MUL", self, o)
    def __rmul__(self, o): return _binary("MUL", o, self)
    def __truediv__(self, o): return _binary("DIV", self, o)
    def __rtruediv__(self, o): return _binary("DIV", o, self)
    def __pow__(self, o): return _binary("POW", self, o)
    def __rpow__(self, o): return _binary("POW", o, self)
    def __neg__(self): return self.tr.emit("NEG", self)
    def __pos__(self): return self
    def __abs__(self): return self.tr.emit("ABS", self)

    __bool__ = _no_value("branches on a traced value")
    __float__ = _no_value("converts a traced value to a float")
    __int__ = _no_value("converts a traced value to an int")
    __index__ = _no_value("uses a traced value as an index")
    __lt__ = __le__ = __gt__ = __ge__ = _no_value("compares a traced value")
    __eq__ = __ne__ = _no_value("compares a traced value")
    __hash__ = None

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        return _apply_ufunc(ufunc, method, inputs, kwargs)


class _SymVec:
    """The traced input vector y (or an element-wise function of it)."""
    __array_priority__ = 1000.0

    def __init__(self, items):
        self.items = list(items)

    def __len__(self): return len(self.items)
    def __iter__(self): return iter(self.items)

    @property
    def shape(self): return (len(self.items),)

    def __getitem__(self, k):
        if isinstance(k, (int, np.integer)):
            return self.items[k]
        if isinstance(k, slice):
            return _SymVec(self.items[k])
        return _SymVec([self.items[i] for i in np.arange(len(self.items))[k]])

    def sum(self):
        acc = self.items[0]
        for it in self.items[1:]:
            acc = acc + it
        return acc

    def dot(self, w):
        if isinstance(w, _SymVec):                           # two traced vectors (θ[1:] @ x of a mean closure)
            return (self * w).sum()
        w = np.asarray(w, dtype=np.float64)
        if w.shape[0] != len(self.items):
            raise ValueError(f"{_label_of(self)}: y @ w with a weight array of another length")
        if w.ndim == 1:
            return _SymVec([x * float(c) for x, c in zip(self.items, w)]).sum()
        if w.ndim == 2:
            return _SymVec([_SymVec([x * float(c) for x, c in zip(self.items, w[:, k])]).sum() for k in range(w.shape[1])])
        raise ValueError(f"{_label_of(self)}: y @ w takes a vector or a matrix of weights")

    def __matmul__(self, w): return self.dot(w)
    def __rmatmul__(self, w): return _SymVec(self.items).dot(np.asarray(w, dtype=np.float64).T)

    def __add__(self, o): return _binary("ADD", self, o)
    def __radd__(self, o): return _binary("ADD", o, self)
    def __sub__(self, o): return _binary("SUB", self, o)
    def __rsub__(self, o): return _binary("SUB", o, self)
    def __mul__(self, o): return _binary("MUL", self, o)
    def __rmul__(self, o): return _binary("MUL", o, self)
    def __truediv__(self, o): return _binary("DIV", self, o)
    def __rtruediv__(self, o): return _binary("DIV", o, self)
    def __pow__(self, o): return _binary("POW", self, o)
    def __rpow__(self, o): return _binary("POW", o, self)
    def __neg__(self): return _SymVec([-x for x in self.items])
    def __pos__(self): return self
    def __abs__(self): return _SymVec([abs(x) for x in self.items])

    __bool__ = _no_value("branches on the traced vector")
    __lt__ = __le__ = __gt__ = __ge__ = _no_value("compares the traced vector")
    __eq__ = __ne__ = _no_value("compares the traced vector")
    __hash__ = None

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        return _apply_ufunc(ufunc, method, inputs, kwargs)

    def __array_function__(self, func, types, args, kwargs):
        if func is np.sum and len(args) == 1 and not kwargs:
            return args[0].sum()
        if func is np.dot and len(args) == 2 and not kwargs:
            a, b = args
            return a.dot(b) if isinstance(a, _SymVec) else b.__rmatmul__(a)
        raise ValueError(f"{_label_of(self, *args)}: np.{getattr(func, '__name__', func)} is not supported in a device {_noun_of(self, *args)}")


def _tracer_of(*xs):
    for x in xs:
        if isinstance(x, _Sym):
            return x.tr
        if isinstance(x, _SymVec):
            return x.items[0].tr
    raise AssertionError


def _scalar_binary(tr, op, a, b):
    if op == "POW" and not isinstance(b, (_Sym, _SymVec)) and float(b) == 2.0:
        return tr.emit("SQUARE", a)
    return tr.emit(op, a, b)


def _binary(op, a, b):
    tr = _tracer_of(a, b)
    vec = [x for x in (a, b) if isinstance(x, _SymVec) or (isinstance(x, (np.ndarray, list, tuple)) and np.ndim(x) == 1)]
    if not vec:
        return _scalar_binary(tr, op, a, b)
    n = len(vec[0])

    def item(x, k):
        if isinstance(x, _SymVec) or (isinstance(x, (np.ndarray, list, tuple)) and np.ndim(x) == 1):
            if len(x) != n:
                raise ValueError(f"{tr.label}: element-wise operation on vectors of different lengths")
            return x[k]
        return x
    return _SymVec([_scalar_binary(tr, op, item(a, k), item(b, k)) for k in range(n)])


def _apply_ufunc(ufunc, method, inputs, kwargs):
    ops = _UFUNC_OPS
    extra = next((getattr(x.tr if isinstance(x, _Sym) else x.items[0].tr, "extra_ufuncs", None) for x in inputs
                  if isinstance(x, _Sym) or (isinstance(x, _SymVec) and x.items)), None)
    if extra:                                                # (the tracer of a DeviceAcquisition also knows scipy.special.ndtr, acq_program.py)
        ops = {**_UFUNC_OPS, **extra}
    if method != "__call__" or kwargs or ufunc not in ops:
        raise ValueError(f"{_label_of(*inputs)}: np.{ufunc.__name__}{'' if method == '__call__' else '.' + method} is not supported in a "
                         f"device {_noun_of(*inputs)} (supported: {', '.join(sorted(u.__name__ for u in ops))})")
    op = ops[ufunc]
    if len(inputs) == 2:
        return _binary(op, inputs[0], inputs[1])
    x = inputs[0]
    if isinstance(x, _SymVec):
        return _SymVec([it.tr.emit(op, it) for it in x.items])
    return x.tr.emit(op, x)


def trace_fitness(fitness: Callable, y_dim: int) -> api.FitnessProgram:
    """Trace `fitness` on y_dim symbolic inputs and check the program against the closure.  ValueError names what failed."""
    P = int(y_dim)
    if P < 1 or P > api.FIT_MAX_INPUTS:
        raise ValueError(f"DeviceFitness: y_dim = {P}, a fitness program takes 1 to {api.FIT_MAX_INPUTS} inputs")
    tr = _Tracer(P)
    out = fitness(_SymVec([_Sym(tr, ("y", p)) for p in range(P)]))
    if isinstance(out, _SymVec) and len(out) == 1:
        out = out[0]
    if isinstance(out, np.ndarray) and out.size == 1:
        out = out.reshape(-1)[0]
    if not isinstance(out, _Sym):
        try:
            out = tr.sym(out)                                # a closure that ignores its input: a constant program
        except ValueError:
            raise ValueError(f"DeviceFitness: the closure must return one scalar, it returned {type(out).__name__}") from None
    prog = tr.program(out)
    Y = np.random.default_rng(0).standard_normal((P, 8))
    with np.errstate(all="ignore"):
        want = np.array([float(fitness(Y[:, k].copy())) for k in range(8)])
    got = prog.eval(Y)
    ok = (np.isnan(want) & np.isnan(got)) | (np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))) | (got == want)
    if not np.all(ok):
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"DeviceFitness: the traced program disagrees with the closure at a test point (closure {want[k]!r}, program "
                         f"{got[k]!r}): the closure does something the trace did not see")
    return prog


class DeviceFitness(NonlinFitness):
    """NonlinFitness(fitness) whose Expected Improvement runs on the device.  Every isinstance(…, NonlinFitness) check and the host
    path keep working; calling it calls the original closure.  `program` is the traced api.FitnessProgram."""

    def __init__(self, fitness: Callable, y_dim: int):
        super().__init__(fitness)
        self.y_dim = int(y_dim)
        self.program = trace_fitness(fitness, y_dim)
