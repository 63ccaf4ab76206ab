"""HipTransformedModel — TransformedModel (src/models/transformed.jl): a base model behind an input warp x -> x_ and an output
transform (y_, std_) -> (y, std) with backward: y -> y_.

Two kinds of transforms:
  InputTransform / JointOutputTransform / SlicedOutputTransform   plain closures with the reference's semantics on the host,
        column by column (transformed.jl:229-297).  A closure has no derivative here: HipGradientAM refuses them.
  DeviceInputTransform / DeviceOutputTransform / DeviceSlicedOutputTransform   the same closures traced ONCE into straight-line
        programs (the rules, limits and 8-point self-check of DeviceMean, mean.py).  A model whose transforms are all of this kind
        carries an api.WarpProgram: candidates are warped on the device, the handles predict in model space, the moments and their
        gradients go through the output programs and both Jacobians on the device, and the EI × feasibility epilogue runs on the
        user-space result — one call (boss_warp_predict[_grad], boss_acq_ei[_grad]_warp).
`backward` stays a host closure either way: it runs once per fit on the data (transformed.jl:222-257).

Base models: HipGaussianProcess, and HipGradientGaussianProcess with traced transforms (its gradient observations are carried to model
space with the transforms' Jacobians, HipTransformedModel._transform_gradient_data).

Parameters are the base model's own (the reference's TransformedParams only wraps them): fitters fit the base model on the
transformed data (base_problem).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np

from . import api
from .mean import device_mean_of, trace_mean
from .problem import ExperimentData, NonlinFitness, best_so_far, in_bounds, in_cons


def _trace(label: str, closure: Callable, n_in: int, n_out: int) -> api.MeanProgram:
    """trace_mean with T = 0, its messages speaking for `label`."""
    try:
        return trace_mean(closure, n_in, 0, n_out)
    except ValueError as e:
        raise ValueError(str(e).replace("DeviceMean", label)) from None


def _cols(X):
    X = np.asarray(X, float)
    return X[:, None] if X.ndim == 1 else X


# ---------------------------------------------------------------------------------------------- transforms
class InputTransform:
    """InputTransform(forward) (transformed.jl:12-14): forward maps one point x to x_."""

    def __init__(self, forward: Callable):
        self.forward = forward

    def __call__(self, x):
        return self.forward(x)

    def apply(self, X):
        """_transform_input_forward (transformed.jl:229-242): a vector as it is, a matrix column by column."""
        X = np.asarray(X, float)
        if X.ndim == 1:
            return np.asarray(self.forward(X), float).reshape(-1)
        return np.stack([np.asarray(self.forward(X[:, j]), float).reshape(-1) for j in range(X.shape[1])], axis=1)


class DeviceInputTransform(InputTransform):
    """InputTransform whose closure has been traced into out_dim programs over x_dim inputs (`program`).  Calling it calls the closure."""

    def __init__(self, forward: Callable, x_dim: int, out_dim: int):
        super().__init__(forward)
        self.x_dim, self.out_dim = int(x_dim), int(out_dim)
        if self.x_dim > api.WARP_MAX_DIM:
            raise ValueError(f"DeviceInputTransform: x_dim = {self.x_dim}, a warp takes x_dim <= {api.WARP_MAX_DIM}")
        self.program = _trace("DeviceInputTransform", forward, self.x_dim, self.out_dim)


class JointOutputTransform:
    """JointOutputTransform(forward, backward) (transformed.jl:54-57): forward(y_, std_) -> (y, std) and backward(y) -> y_ over
    vectors of all outputs."""

    def __init__(self, forward: Callable, backward: Callable):
        self.forward, self.backward = forward, backward

    def forward_cols(self, mu_, sd_):
        """_transform_output_forward (transformed.jl:263-265,279-286): P-vectors as they are, P×M matrices column by column."""
        mu_, sd_ = np.asarray(mu_, float), np.asarray(sd_, float)
        if mu_.ndim == 1:
            m, s = self.forward(mu_, sd_)
            return np.asarray(m, float).reshape(-1), np.asarray(s, float).reshape(-1)
        mu, sd = np.empty_like(mu_), np.empty_like(sd_)
        for k in range(mu_.shape[1]):
            m, s = self.forward(mu_[:, k], sd_[:, k])
            mu[:, k], sd[:, k] = np.asarray(m, float).reshape(-1), np.asarray(s, float).reshape(-1)
        return mu, sd

    def backward_cols(self, Y):
        """_transform_output_backward (transformed.jl:248-250)."""
        Y = np.asarray(Y, float)
        return np.stack([np.asarray(self.backward(Y[:, j]), float).reshape(-1) for j in range(Y.shape[1])], axis=1)


class SlicedOutputTransform:
    """SlicedOutputTransform(forward, backward) (transformed.jl:90-102): forward[i](y_i_, std_i_) -> (y_i, std_i) and
    backward[i](y_i) -> y_i_ over scalars, one pair per output."""

    def __init__(self, forward: Sequence[Callable], backward: Sequence[Callable]):
        if len(forward) != len(backward):
            raise ValueError("Forward and backward function arrays must have the same length.")
        self.forward, self.backward = list(forward), list(backward)

    def slice(self, idx: int) -> "SlicedOutputTransform":
        return SlicedOutputTransform([self.forward[idx]], [self.backward[idx]])

    def forward_cols(self, mu_, sd_):
        """_transform_output_forward (transformed.jl:266-273,287-297)."""
        mu_, sd_ = np.asarray(mu_, float), np.asarray(sd_, float)
        mu, sd = np.empty_like(mu_), np.empty_like(sd_)
        for i, f in enumerate(self.forward):
            if mu_.ndim == 1:
                mu[i], sd[i] = f(mu_[i], sd_[i])
            else:
                for k in range(mu_.shape[1]):
                    mu[i, k], sd[i, k] = f(mu_[i, k], sd_[i, k])
        return mu, sd

    def backward_cols(self, Y):
        """_transform_output_backward (transformed.jl:251-257)."""
        Y = np.asarray(Y, float)
        out = np.empty_like(Y)
        for i, f in enumerate(self.backward):
            out[i, :] = [f(v) for v in Y[i, :]]
        return out


def _as_list(a):
    return list(a) if isinstance(a, (list, tuple, np.ndarray)) or hasattr(a, "items") else [a]


def _check_backward(label: str, tr, P: int):
    """forward(backward(y), ·)[0] ≈ y at 8 random points, else ValueError."""
    rng = np.random.default_rng(1)
    Y = rng.standard_normal((P, 8))
    with np.errstate(all="ignore"):
        got = tr.forward_cols(tr.backward_cols(Y), np.full((P, 8), 0.5))[0]
    ok = np.abs(got - Y) <= 1e-8 * np.maximum(1.0, np.abs(Y))
    if not np.all(ok):
        p, k = (int(i[0]) for i in np.nonzero(~ok))
        raise ValueError(f"{label}: forward(backward(y)) does not return y (output {p}: y = {Y[p, k]!r}, forward(backward(y)) = "
                         f"{got[p, k]!r}): backward is not the inverse of forward's mean")


class DeviceOutputTransform(JointOutputTransform):
    """JointOutputTransform whose forward has been traced into 2·y_dim programs over (y_, std_) (`program`)."""

    def __init__(self, forward: Callable, backward: Callable, y_dim: int):
        super().__init__(forward, backward)
        self.y_dim = P = int(y_dim)
        if P < 1 or P > api.WARP_MAX_OUTPUTS:
            raise ValueError(f"DeviceOutputTransform: y_dim = {P}, an output program has 1 to {api.WARP_MAX_OUTPUTS} outputs")

        def packed(z):
            m, s = forward(z[:P], z[P:])
            return _as_list(m) + _as_list(s)
        self.program = _trace("DeviceOutputTransform", packed, 2 * P, 2 * P)
        _check_backward("DeviceOutputTransform", self, P)


class DeviceSlicedOutputTransform(SlicedOutputTransform):
    """SlicedOutputTransform whose scalar closures have been traced and packed into the joint form (`program`): output i reads
    (y_i_, std_i_) alone, so every cross-derivative of the programs is an exact zero."""

    def __init__(self, forward: Sequence[Callable], backward: Sequence[Callable]):
        super().__init__(forward, backward)
        self.y_dim = P = len(self.forward)
        if P < 1 or P > api.WARP_MAX_OUTPUTS:
            raise ValueError(f"DeviceSlicedOutputTransform: {P} outputs, an output program has 1 to {api.WARP_MAX_OUTPUTS}")

        def packed(z):
            pairs = [f(z[i], z[P + i]) for i, f in enumerate(self.forward)]
            return [a for a, _ in pairs] + [b for _, b in pairs]
        self.program = _trace("DeviceSlicedOutputTransform", packed, 2 * P, 2 * P)
        _check_backward("DeviceSlicedOutputTransform", self, P)

    def slice(self, idx: int) -> "DeviceSlicedOutputTransform":
        return DeviceSlicedOutputTransform([self.forward[idx]], [self.backward[idx]])


_DEVICE_KINDS = (DeviceInputTransform, DeviceOutputTransform, DeviceSlicedOutputTransform)


# ---------------------------------------------------------------------------------------------- the model
@dataclass
class HipTransformedModel:
    """TransformedModel(base_model, input_transform, output_transform) (transformed.jl:127-134) over a HipGaussianProcess or a
    HipGradientGaussianProcess.  With both transforms None every result is the base model's.
    A HipGradientGaussianProcess is fitted on GradientData: its gradient observations ∂y/∂x must reach the base model as ∂y_/∂x_ =
    (∂y/∂y_)⁻¹ · ∂y/∂x · (∂x_/∂x)⁻¹, which takes the Jacobians of both transforms — so over that base model every given transform
    must be a traced one (a plain closure has no derivative) and the input warp must keep the dimension (a square ∂x_/∂x)."""
    base_model: object
    input_transform: Optional[InputTransform] = None
    output_transform: object = None

    def __post_init__(self):
        from .gradient_gp import HipGradientGaussianProcess
        from .model import HipGaussianProcess
        if type(self.base_model) not in (HipGaussianProcess, HipGradientGaussianProcess):
            raise NotImplementedError(f"HipTransformedModel wraps a HipGaussianProcess or a HipGradientGaussianProcess; "
                                      f"{type(self.base_model).__name__} as the base model is not supported")
        from .kernel import refuse_device_kernel
        refuse_device_kernel(self.base_model, "HipTransformedModel over such a base model (the warped calls are built-in-kernel only)")
        it, ot = self.input_transform, self.output_transform
        self.gradient_base = type(self.base_model) is HipGradientGaussianProcess
        if it is not None and not isinstance(it, InputTransform):
            raise ValueError("input_transform must be an InputTransform, a DeviceInputTransform or None")
        if ot is not None and not isinstance(ot, (JointOutputTransform, SlicedOutputTransform)):
            raise ValueError("output_transform must be a JointOutputTransform, a SlicedOutputTransform, their Device twins or None")
        P = self.base_model.y_dim
        if isinstance(ot, SlicedOutputTransform) and len(ot.forward) != P:
            raise ValueError(f"the output transform has {len(ot.forward)} slices, the base model {P} outputs")
        if isinstance(ot, DeviceOutputTransform) and ot.y_dim != P:
            raise ValueError(f"the output transform was traced with y_dim = {ot.y_dim}, the base model has {P} outputs")
        given = [t for t in (it, ot) if t is not None]
        if self.gradient_base:
            if not all(isinstance(t, _DEVICE_KINDS) for t in given):
                raise NotImplementedError("HipTransformedModel over a HipGradientGaussianProcess needs traced transforms (DeviceInputTransform, "
                                          "DeviceOutputTransform, DeviceSlicedOutputTransform): the gradient observations are carried to "
                                          "model space with the transforms' Jacobians, and a plain closure has no derivative")
            if it is not None and it.x_dim != it.out_dim:
                raise ValueError(f"HipTransformedModel over a HipGradientGaussianProcess: the input warp maps {it.x_dim} to {it.out_dim} "
                                 "dimensions; gradient observations need a square, invertible ∂x_/∂x")
        self.warp = None                                     # api.WarpProgram when every given transform is a traced one
        if given and all(isinstance(t, _DEVICE_KINDS) for t in given):
            self.warp = api.WarpProgram(None if it is None else it.program, P, None if ot is None else ot.program)

    @property
    def device(self):
        return self.base_model.device

    @property
    def y_dim(self):
        return self.base_model.y_dim

    @property
    def sliceable(self):
        """transformed.jl:178-180: the base model's, and never under a joint output transform."""
        return bool(self.base_model.sliceable) and not isinstance(self.output_transform, JointOutputTransform)

    def params_sampler(self):
        return self.base_model.params_sampler()

    def params_loglike(self):
        return self.base_model.params_loglike()

    def vectorizer(self, *a, **k):
        return self.base_model.vectorizer(*a, **k)

    def transform_data(self, data: ExperimentData) -> ExperimentData:
        """_transform_data (transformed.jl:222-226): X forward, Y backward."""
        if self.input_transform is None and self.output_transform is None:
            return data
        X_ = data.X if self.input_transform is None else self.input_transform.apply(data.X)
        Y_ = data.Y if self.output_transform is None else self.output_transform.backward_cols(data.Y)
        if self.gradient_base:
            return self._transform_gradient_data(data, X_, Y_)
        return ExperimentData(np.asfortranarray(X_), np.ascontiguousarray(Y_))

    def _transform_gradient_data(self, data, X_, Y_):
        """GradientData to model space: dY_[:, :, j] = A_j⁻¹ · dY[:, :, j] · J_j⁻¹ with J_j = ∂x_/∂x at x_j (the input program's reverse
        sweep, on the host) and A_j = ∂y/∂y_ at y_j_ (the mean rows of the output program; the check at construction made them
        independent of std_, which is taken as 1 here).  The inverse-function theorem stands in for a derivative of `backward`."""
        from .gradient_gp import GradientData
        it, ot = self.input_transform, self.output_transform
        P, n = Y_.shape
        dY = np.asarray(data.dY, float)                      # [P, d, n]
        out = np.empty_like(dY)
        J = None if it is None else api.WarpProgram(it.program, P, None).apply_host(data.X, True)[1]          # [n, d, d]
        A = None
        if ot is not None:
            A = ot.program.jac(np.vstack([Y_, np.ones_like(Y_)]))[1][0, :P, :P, :]                               # [P, P, n]
        for j in range(n):
            G = dY[:, :, j]
            if A is not None:
                G = np.linalg.solve(A[:, :, j], G)
            if J is not None:
                G = np.linalg.solve(J[j].T, G.T).T           # G · J⁻¹
            out[:, :, j] = G
        return GradientData(np.asfortranarray(X_), np.ascontiguousarray(Y_), out)

    def data_loglike(self, data: ExperimentData):
        return self.base_model.data_loglike(self.transform_data(data))

    def data_loglike_batch(self, data: ExperimentData, samples):
        return self.base_model.data_loglike_batch(self.transform_data(data), samples)

    def data_loglike_grad_batch(self, data: ExperimentData, plist):
        return self.base_model.data_loglike_grad_batch(self.transform_data(data), plist)

    def model_posterior(self, params, data: ExperimentData, reserve: int = 0):
        """model_posterior (transformed.jl:211-219): the base model's posterior of the transformed data behind the transforms."""
        if reserve:
            raise NotImplementedError("HipTransformedModel: appending observations to a transformed posterior is not supported")
        base = self.base_model.model_posterior(params, self.transform_data(data))      # (both base models take these two arguments)
        if isinstance(base, list):
            return [HipTransformedPosterior(self, b) for b in base]
        return HipTransformedPosterior(self, base)


def base_problem(problem):
    """The problem a fitter works on: a HipTransformedModel's base model over the transformed data (its parameters are the base
    model's); any other problem as it is."""
    if not isinstance(problem.model, HipTransformedModel):
        return problem
    prob = copy.copy(problem)
    prob.model = problem.model.base_model
    prob.data = problem.model.transform_data(problem.data)
    return prob


def _prior_means(posts, X, jac_x: bool = False):
    """(S×P×M prior means of the base model at the WARPED points, S×P×d_model×M ∂m/∂x_ or None), or (None, None) without a prior
    mean.  The warped points come from boss_warp_apply where the model carries a warp program (the one-call paths warp their own
    copy on the device), else from the closure."""
    model = posts[0].model
    base = model.base_model
    if model.gradient_base or (base.mean is None and base.parametric is None):      # (the gradient model's posterior uses no mean)
        return None, None
    if model.input_transform is None:
        X_ = X
    elif model.warp is not None:
        X_ = model.warp.apply(X, device=model.device)[0]
    else:
        X_ = model.input_transform.apply(X)
    if device_mean_of(base) is not None:
        m, _, jx = base.device_means(X_, [p.base.slices[0].params for p in posts], api.MEAN_SAMPLE_MAJOR, jac_x=jac_x)
        return m, jx
    if jac_x and (callable(base.mean) or base.parametric is not None):
        raise NotImplementedError("HipGradientAM over a transformed model needs the base model's prior mean as a DeviceMean (or a "
                                  "constant): a closure has no derivative")
    return np.stack([np.stack([s._mean_s(X_) for s in p.base.slices]) for p in posts]), None


class HipTransformedPosterior:
    """TransformedPosterior (transformed.jl:160-167, 302-378)."""

    def __init__(self, model: HipTransformedModel, base):
        self.model, self.base = model, base

    @property
    def slices(self):
        return self.base.slices

    def _identity(self):
        return self.model.input_transform is None and self.model.output_transform is None

    def mean_and_var(self, x):
        if self._identity():
            return self.base.mean_and_var(x)
        x = np.asarray(x, float)
        if self.model.warp is not None:
            X = _cols(x)
            mu, var = self.model.warp.predict([[s.gp for s in self.base.slices]], X, _prior_means([self], X)[0])
            return (mu[0, :, 0], var[0, :, 0]) if x.ndim == 1 else (mu[0], var[0])
        it, ot = self.model.input_transform, self.model.output_transform
        mu_, var_ = self.base.mean_and_var(x if it is None else it.apply(x))
        if ot is None:
            return mu_, var_
        mu, sd = ot.forward_cols(mu_, np.sqrt(var_))
        return mu, sd ** 2

    def mean(self, x):
        return self.mean_and_var(x)[0]

    def var(self, x):
        return self.mean_and_var(x)[1]

    def std(self, x):
        return np.sqrt(self.var(x))

    def mean_and_std(self, x):
        mu, var = self.mean_and_var(x)
        return mu, np.sqrt(var)

    def mean_and_var_grad(self, X):
        """(mu[P, M], var[P, M], dmu[P, d, M], dvar[P, d, M]) w.r.t. the user-space columns of X, on the device."""
        X = _cols(X)
        if self.model.warp is None:
            raise NotImplementedError("mean_and_var_grad needs traced transforms (DeviceInputTransform, DeviceOutputTransform, "
                                      "DeviceSlicedOutputTransform): a plain closure has no derivative")
        ms, mg = _prior_means([self], X, jac_x=True)
        mu, var, dmu, dvar = self.model.warp.predict_grad([[s.gp for s in self.base.slices]], X, ms, mg)
        return mu[0], var[0], dmu[0], dvar[0]

    def mean_and_cov(self, X):
        """transformed.jl:353-378: the base covariances with their diagonals replaced under a sliced transform; a joint one has no
        covariance."""
        it, ot = self.model.input_transform, self.model.output_transform
        if isinstance(ot, JointOutputTransform):
            raise RuntimeError("Cannot compute covariance with joint output transform. Use mean_and_var instead.")
        X = np.asarray(X, float)
        mu_, cov = self.base.mean_and_cov(X if it is None else it.apply(X))
        if ot is None:
            return mu_, cov
        idx = np.arange(cov.shape[0])
        mu, sd = ot.forward_cols(mu_, np.sqrt(cov[idx, idx, :].T))
        cov = cov.copy()
        cov[idx, idx, :] = (sd ** 2).T
        return mu, cov

    def cov(self, X):
        return self.mean_and_cov(X)[1]

    def append(self, x, y):
        raise NotImplementedError("HipTransformedModel: appending observations to a transformed posterior is not supported")

    def close(self):
        self.base.close()


# ---------------------------------------------------------------------------------------------- what the maximizers call
def _acq_args(problem, X):
    ei = problem.acquisition
    if isinstance(ei.fitness, NonlinFitness):
        raise NotImplementedError("a transformed model needs the analytic EI of LinFitness (NonlinFitness / DeviceFitness over a "
                                  "warped model is not supported)")
    b = best_so_far(ei.fitness, problem.data.Y, problem.y_max)          # user space, as in the reference
    mask = (in_bounds(X, problem.domain.bounds) & in_cons(X, problem.domain.cons)) if ei.cons_safe else None
    return ei.fitness.coefs, b, mask


def warped_acquisition_values(problem, posts, Xs):
    """acquisition_values for HipTransformedPosteriors: (acq[M], argmax, max).  Traced transforms: one boss_acq_ei_warp call;
    plain closures: the posteriors' host path, then the epilogue on the user-space moments (boss_acq_ei_moments)."""
    coefs, b, mask = _acq_args(problem, Xs)
    model = problem.model
    if model.warp is None:
        mv = [p.mean_and_var(Xs) for p in posts]
        return api.acq_ei_moments(np.stack([m for m, _ in mv]), np.stack([v for _, v in mv]), coefs, problem.y_max, b, mask, model.device)
    gps = [[s.gp for s in p.base.slices] for p in posts]
    return model.warp.acq_ei(gps, Xs, coefs, problem.y_max, b, mask, _prior_means(posts, Xs)[0])


def warped_value_and_grad(problem, posts, X):
    """HipGradientAM's value and gradient for HipTransformedPosteriors: one boss_acq_ei_grad_warp call."""
    coefs, b, mask = _acq_args(problem, X)
    model = problem.model
    if model.warp is None:
        raise NotImplementedError("HipGradientAM needs traced transforms (DeviceInputTransform, DeviceOutputTransform, "
                                  "DeviceSlicedOutputTransform): a plain closure has no derivative")
    gps = [[s.gp for s in p.base.slices] for p in posts]
    ms, mg = _prior_means(posts, X, jac_x=True)
    return model.warp.acq_ei_grad(gps, X, coefs, problem.y_max, b, mask, ms, mg)
