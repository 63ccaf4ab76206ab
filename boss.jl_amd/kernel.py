"""DeviceKernel — a user-defined covariance function (KernelFunctions.Kernel / CustomKernel(f), src/models/utils/kernels.jl:3-13)
traced once into a straight-line program over two points (api.KernelProgram, boss_kern_t), so that a GaussianProcess can carry any
kernel the reference's finite_gp accepts (src/models/gaussian_process.jl:239-243):  k(x, y) = (α+1e-8)² f(u, v)  with
u = x ⊘ (λ+1e-8), v = y ⊘ (λ+1e-8) — an exponential, rational-quadratic, periodic, sum, product or dot-product kernel.  The Gram
matrix, the cross-covariances and the per-candidate prior variance f(u*, u*) are then evaluated by the program on the device
(boss_kgp_create).

The closure f(u, v) is called ONCE on two symbolic length-d vectors, with the rules of DeviceFitness (fitness.py: arithmetic, the
listed numpy functions, indexing, slicing, sum, dot; no data-dependent control flow, math.*, float()), and returns one scalar.
Limits: x_dim <= 16 (32 inputs), 32 constants, 64 instructions.  The traced program is checked at 8 seeded point pairs: against the
closure, and for symmetry — f(u, v) and f(v, u) may differ by 16 ulp of |f|, or of the largest |f| over the test pairs where f is
smaller than that (the order of a sum), an asymmetric function is not a kernel.  Hyper-parameters beyond λ, α, σ (the shape of a
rational-quadratic kernel, a period) are traced constants.

DeviceKernel(f, x_dim, grad=True) switches the model's gradients on (boss_kgp_set_grad): mean_and_var_grad, data_loglike_grad_batch,
HipGradientMAP, HipSampleOptMAP and HipGradientAM then work as for a built-in kernel.  Tracing then also checks the DERIVATIVE
program (api.KernelProgram.grad, the reverse sweep the gradient kernels run): at the 8 seeded pairs every partial ∂f/∂u, ∂f/∂v must be
finite and agree with central differences of the closure (h = 1e-5) within 1e-6·max(1, |∂f|) — truncation is of order h², rounding of
order ε/h, both far below that —, and at 8 coincident pairs (u, u) every partial must be finite (a one-sided cusp has no central
difference to agree with; the sweep passes a local partial of exactly 0 on as 0, which is what makes exp(-sqrt(r2)) finite there).

DeviceKernel(f, x_dim, sequential=True) switches appends and tracked candidates on (boss_kgp_set_sequential), independently of grad:
slice.append, post.append, model_posterior(..., reserve=…) and HipSequentialBatchAM (tracked candidates or the untracked loop) then
work as for a built-in kernel.  Covariances, devices=[…], warps and the gradient-observation / nonstationary models stay refused.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from . import api
from .fitness import _Sym, _SymVec, _Tracer

_LABEL = "DeviceKernel"
_SYM_ULPS = 16.0                                             # |f(u, v) − f(v, u)| <= 16 · 2⁻⁵² · |f|: re-ordered sums and products


_FD_H, _FD_TOL = 1e-5, 1e-6


def _check_derivative(closure: Callable, prog: api.KernelProgram, U, V):
    """The grad=True validation of the derivative program (module docstring).  ValueError names what failed."""
    d = prog.d
    _, dU, dV = prog.grad(U, V)
    _, cU, cV = prog.grad(U, U)
    for what, arrs in (("a test pair", (dU, dV)), ("a coincident pair (u, u)", (cU, cV))):
        for side, a in zip("uv", arrs):
            if not np.all(np.isfinite(a)):
                m, k = (int(i[0]) for i in np.nonzero(~np.isfinite(a)))
                raise ValueError(f"{_LABEL}: grad=True, but the derivative program gives ∂f/∂{side}[{m}] = {a[m, k]!r} at {what}: "
                                 "every partial must be finite")
    with np.errstate(all="ignore"):
        for k in range(U.shape[1]):
            for side, got in (("u", dU), ("v", dV)):
                for m in range(d):
                    pts = []
                    for sgn in (1.0, -1.0):
                        u, v = U[:, k].copy(), V[:, k].copy()
                        (u if side == "u" else v)[m] += sgn * _FD_H
                        pts.append(float(closure(u, v)))
                    fd = (pts[0] - pts[1]) / (2.0 * _FD_H)
                    if not abs(got[m, k] - fd) <= _FD_TOL * max(1.0, abs(got[m, k])):
                        raise ValueError(f"{_LABEL}: grad=True, but the derivative program disagrees with the closure's central "
                                         f"differences at a test pair (∂f/∂{side}[{m}]: program {got[m, k]!r}, differences {fd!r})")


def trace_kernel(closure: Callable, x_dim: int, grad: bool = False) -> api.KernelProgram:
    """Trace `closure` on two symbolic points of x_dim entries and check the program — with grad=True its derivative program too.
    ValueError names what failed."""
    d = int(x_dim)
    if d < 1 or d > api.KERN_MAX_DIM:
        raise ValueError(f"{_LABEL}: x_dim = {d}, a kernel program takes two points of 1 to {api.KERN_MAX_DIM} dimensions")
    tr = _Tracer(2 * d, _LABEL, "kernel")
    out = closure(_SymVec([_Sym(tr, ("y", k)) for k in range(d)]), _SymVec([_Sym(tr, ("y", d + k)) for k in range(d)]))
    if isinstance(out, _SymVec) and len(out) == 1:
        out = out[0]
    if isinstance(out, np.ndarray) and out.size == 1:
        out = out.reshape(-1)[0]
    if not isinstance(out, _Sym):
        try:
            out = tr.sym(out)                                # a closure that ignores its inputs: a constant kernel
        except ValueError:
            raise ValueError(f"{_LABEL}: the closure must return one scalar, it returned {type(out).__name__}") from None
    nc = len(tr.consts)
    if nc > api.FIT_MAX_CONSTS:
        raise ValueError(f"{_LABEL}: the closure needs {nc} constants, a kernel program holds at most {api.FIT_MAX_CONSTS}")
    if len(tr.code) > api.FIT_MAX_INSTR:
        raise ValueError(f"{_LABEL}: the closure traces into {len(tr.code)} instructions, a kernel program holds at most "
                         f"{api.FIT_MAX_INSTR}")

    def vid(ref):
        kind, k = ref
        return k if kind == "y" else tr.P + k if kind == "c" else tr.P + nc + k
    code = [(api.FIT_OP[op], vid(a), -1 if b is None else vid(b)) for op, a, b in tr.code]
    prog = api.KernelProgram(d, tr.consts, np.asarray(code, dtype=np.intc).reshape(-1, 3), vid(out.ref))
    rng = np.random.default_rng(0)
    U, V = rng.standard_normal((d, 8)), rng.standard_normal((d, 8))
    with np.errstate(all="ignore"):
        want = np.array([float(closure(U[:, k].copy(), V[:, k].copy())) for k in range(8)])
    got, swapped = prog.eval(U, V), prog.eval(V, U)
    ok = (np.isnan(want) & np.isnan(got)) | (np.abs(got - want) <= 1e-9 * np.maximum(1.0, np.abs(want))) | (got == want)
    if not np.all(ok):
        k = int(np.flatnonzero(~ok)[0])
        raise ValueError(f"{_LABEL}: the traced program disagrees with the closure at a test point (closure {want[k]!r}, program "
                         f"{got[k]!r}): the closure does something the trace did not see")
    # relative to |f| at the pair, but no finer than the kernel's own size over the test pairs: where f passes through zero (a dot
    # product plus a negative constant) a re-ordered sum differs by ulps of its terms, not of the tiny result
    with np.errstate(all="ignore"):
        size = np.nanmax(np.abs(np.concatenate([got, swapped]))) if np.any(np.isfinite(got)) else 0.0
    floor = size if np.isfinite(size) else 0.0
    sym = (np.isnan(got) & np.isnan(swapped)) | (got == swapped) | \
          (np.abs(got - swapped) <= _SYM_ULPS * np.finfo(float).eps * np.maximum(np.abs(got), floor))
    if not np.all(sym):
        k = int(np.flatnonzero(~sym)[0])
        raise ValueError(f"{_LABEL}: the closure is not symmetric (f(u, v) = {got[k]!r}, f(v, u) = {swapped[k]!r} at a test point): "
                         "an asymmetric function is not a kernel")
    if grad:
        _check_derivative(closure, prog, U, V)
    return prog


class DeviceKernel:
    """The covariance closure with its traced program: HipGaussianProcess(kernel=DeviceKernel(f, x_dim)).  Calling it calls the
    original closure.  `program` is the api.KernelProgram.  grad=True: the model's handles carry gradients; sequential=True: they take
    appends and tracked candidates (module docstring)."""

    def __init__(self, closure: Callable, x_dim: int, grad: bool = False, sequential: bool = False):
        self.closure = closure
        self.x_dim = int(x_dim)
        self.grad = bool(grad)
        self.sequential = bool(sequential)
        self.program = trace_kernel(closure, x_dim, self.grad)

    def __call__(self, u, v):
        return self.closure(u, v)


def device_kernel_of(model) -> Optional[DeviceKernel]:
    """The DeviceKernel a model carries as its kernel, or None (a built-in kernel name)."""
    k = getattr(model, "kernel", None)
    return k if isinstance(k, DeviceKernel) else None


def refuse_device_kernel(model, what: str, grad_ok: bool = False, seq_ok: bool = False):
    """NotImplementedError for the parts of the plugin surface a DeviceKernel model does not reach.  grad_ok: the part needs only
    gradients, which DeviceKernel(..., grad=True) provides; seq_ok: it needs only appends / tracked candidates, which
    DeviceKernel(..., sequential=True) provides."""
    dk = device_kernel_of(model)
    if dk is None or (grad_ok and dk.grad) or (seq_ok and dk.sequential):
        return
    if grad_ok:
        raise NotImplementedError(f"{what} is not available for a model whose kernel is a DeviceKernel traced without gradients: "
                                  "DeviceKernel(f, x_dim, grad=True) switches candidate / likelihood gradients on")
    if seq_ok:
        raise NotImplementedError(f"{what} is not available for a model whose kernel is a plain DeviceKernel: "
                                  "DeviceKernel(f, x_dim, sequential=True) switches appends and tracked candidates on")
    raise NotImplementedError(f"{what} is not available for a model whose kernel is a DeviceKernel (a traced program kernel has no "
                              "covariances, warps or in-library multi-device path yet)")
