"""HipGaussianProcess — the SurrogateModel of the plugin trio (host-side mirror).

Mirrors the reference's GaussianProcess / Semiparametric surface (src/models/gaussian_process.jl,
src/models/semiparametric.jl) over the C ABI:
  model_posterior / model_posterior_slice   -> boss_gp_create + boss_gp_update (resident factor)
  mean / var / mean_and_var / std / ...     -> boss_gp_predict
  data_loglike                              -> boss_gp_update's logpdf (or boss_gp_loglike_batch)
  data_loglike_grad_batch                   -> boss_gp_loglike_grad_batch_mean (values, ∂/∂(λ, α, σ) and, through the
                                               Jacobian of the parametric mean, ∂/∂θ)
  params_loglike / params_sampler           -> host (prior bookkeeping, out of the GPU's scope)
The GP's prior mean (a user closure, or the Semiparametric parametric model m(x;θ)) is evaluated
on the host and crosses the ABI as dense vectors — unless it is a DeviceMean (mean.py): then the traced program
gives the mean, ∂m/∂θ and ∂m/∂x of all points, outputs and parameter sets in one device call (boss_mean_eval) and the closure is
never called.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import api
from .kernel import device_kernel_of, refuse_device_kernel
from .mean import DeviceMean, device_mean_of
from .problem import ExperimentData


@dataclass
class HipGPParams:
    """GaussianProcessParams(λ, α, σ) (gaussian_process.jl:62-70) + optional Semiparametric θ."""
    lengthscales: np.ndarray      # d×P
    amplitudes: np.ndarray        # P
    noise_std: np.ndarray         # P
    theta: Optional[np.ndarray] = None

    def __post_init__(self):
        self.lengthscales = np.atleast_2d(np.asarray(self.lengthscales, float))
        self.amplitudes = np.asarray(self.amplitudes, float).reshape(-1)
        self.noise_std = np.asarray(self.noise_std, float).reshape(-1)

    def slice(self, i: int) -> "HipGPParams":
        """slice(::GaussianProcessParams, idx) (gaussian_process.jl:105-111)."""
        return HipGPParams(self.lengthscales[:, i:i + 1], self.amplitudes[i:i + 1], self.noise_std[i:i + 1], self.theta)


def join_slices(ps: Sequence[HipGPParams]) -> HipGPParams:
    """join_slices (gaussian_process.jl:113-119)."""
    return HipGPParams(np.hstack([p.lengthscales for p in ps]), np.concatenate([p.amplitudes for p in ps]),
                       np.concatenate([p.noise_std for p in ps]), ps[0].theta)


@dataclass
class HipGaussianProcess:
    """GaussianProcess(mean, kernel, lengthscale_priors, amplitude_priors, noise_std_priors)
    (gaussian_process.jl:34-42).  `mean`: None, a length-P vector, or a function x -> length-P
    vector.  `parametric`: optional (x, θ) -> length-P vector with `theta_priors` — the
    Semiparametric model (semiparametric.jl:79-92).  `parametric_jac`: optional (x, θ) -> P×T matrix ∂parametric(x, θ)/∂θ for
    the likelihood gradient w.r.t. θ (data_loglike_grad_batch; the reference differentiates the closure by AD).  Without it the
    Jacobian is taken by central differences of `parametric` in θ with step 1e-6·max(1, |θ_t|): 2T further evaluations of
    `parametric` per point; the error is about 2⁻⁵³·|m|/h from rounding plus h²·|∂³m/∂θ³|/6 from truncation.
    `parametric` (or `mean`, with theta_dim = 0) may be a DeviceMean: values and exact Jacobians then come from its traced program on
    the device, and `parametric_jac` is ignored.
    `kernel`: "matern32" | "matern52" | "sqexp", or a DeviceKernel (kernel.py) — a user-defined covariance function traced into a
    device program (boss_kgp_create).  Such a model fits, predicts and drives HipBatchedMAP / HipBatchAM / bo; what needs covariances
    raises NotImplementedError, and so does what needs gradients (mean_and_var_grad, data_loglike_grad_batch, HipGradientMAP,
    HipSampleOptMAP, HipGradientAM) unless the kernel was traced with DeviceKernel(f, x_dim, grad=True), and what needs appends or
    tracked candidates (append, model_posterior(..., reserve=…), HipSequentialBatchAM) unless it was traced with sequential=True."""
    lengthscale_priors: Sequence
    amplitude_priors: Sequence
    noise_std_priors: Sequence
    mean: object = None
    kernel: object = "matern52"                  # default per src/deprecated.jl:34; or a DeviceKernel
    discrete: Optional[Sequence[bool]] = None
    parametric: Optional[Callable] = None
    theta_priors: Optional[Sequence] = None
    device: int = 0
    parametric_jac: Optional[Callable] = None

    sliceable = True                             # gaussian_process.jl:85

    def make_discrete(self, discrete):
        """make_discrete(m, discrete) (gaussian_process.jl:78-79): wrap the kernel in DiscreteKernel."""
        return HipGaussianProcess(self.lengthscale_priors, self.amplitude_priors, self.noise_std_priors, self.mean,
                                  self.kernel, np.asarray(discrete, bool), self.parametric, self.theta_priors, self.device,
                                  self.parametric_jac)

    @property
    def y_dim(self):
        return len(self.amplitude_priors)

    def _new_gp(self, X, y):
        """An unfitted resident handle for one output: boss_gp_create, or boss_kgp_create under a DeviceKernel."""
        dk = device_kernel_of(self)
        if dk is not None:
            return api.KernelGP(X, y, dk.program, self.discrete, self.device, grad=dk.grad, sequential=dk.sequential)
        return api.GP(X, y, self.kernel, self.discrete, self.device)

    # ------------------------------------------------------------------ prior mean on the device (DeviceMean)
    def device_means(self, X, plist: Sequence[Optional[HipGPParams]], layout: int = api.MEAN_SAMPLE_MAJOR, jac_theta: bool = False,
                     jac_x: bool = False):
        """ONE boss_mean_eval for all outputs at the columns of X and the θ of every parameter set of `plist`:
        (m, ∂m/∂θ or None, ∂m/∂x or None) with leading axes (S, P) for layout 0 and (P, S) for layout 1 (api.MeanProgram).  A mean
        without parameters (theta_dim = 0) is evaluated once and repeated along the set axis."""
        dm = device_mean_of(self)
        X = np.asarray(X, float)
        if X.ndim == 1:
            X = X[:, None]
        S = len(plist)
        if dm.theta_dim == 0:
            out = dm.evaluate(X, None, layout, False, jac_x, self.device)
            return tuple(None if a is None else np.repeat(a, S, axis=0 if layout == api.MEAN_SAMPLE_MAJOR else 1) for a in out)
        th = np.stack([np.asarray(p.theta, float).reshape(-1) for p in plist], axis=1)
        if th.shape[0] != dm.theta_dim:
            raise ValueError(f"theta has {th.shape[0]} entries, the DeviceMean was traced with theta_dim = {dm.theta_dim}")
        return dm.evaluate(X, th, layout, jac_theta, jac_x, self.device)

    def mean_values_all(self, X, params: Optional[HipGPParams]):
        """m_i(x_j) of every output as a P×n array (None without a prior mean): one device call with a DeviceMean."""
        if device_mean_of(self) is not None:
            return self.device_means(X, [params])[0][0]
        rows = [self.mean_values(X, params, i) for i in range(self.y_dim)]
        return None if rows[0] is None else np.stack(rows)

    # ------------------------------------------------------------------ prior mean on the host
    def mean_values(self, X, params: Optional[HipGPParams], i: int):
        """m_i(x_j) for all columns j — mean_getindex (gaussian_process.jl:101-103) / parametric(θ)."""
        X = np.asarray(X, float)
        if X.ndim == 1:
            X = X[:, None]
        n = X.shape[1]
        if device_mean_of(self) is not None:
            return np.ascontiguousarray(self.device_means(X, [params])[0][0, i])
        if self.parametric is not None:
            th = params.theta
            return np.array([float(np.asarray(self.parametric(X[:, j], th))[i]) for j in range(n)])
        if self.mean is None:
            return None
        if callable(self.mean):
            return np.array([float(np.asarray(self.mean(X[:, j]))[i]) for j in range(n)])
        return np.full(n, float(np.asarray(self.mean, float)[i]))

    def mean_jacobians(self, X, params: HipGPParams, i: int) -> np.ndarray:
        """∂m_i(x_j; θ)/∂θ_t as an N×T matrix (row j = point j) at params.theta: `parametric_jac` where the model has one, otherwise
        central differences of `parametric` with step 1e-6·max(1, |θ_t|) (2T evaluations per point)."""
        X = np.asarray(X, float)
        if X.ndim == 1:
            X = X[:, None]
        n = X.shape[1]
        th = np.asarray(params.theta, float).reshape(-1)
        T = th.shape[0]
        if isinstance(self.parametric, DeviceMean):          # the exact reverse sweep of the traced program (parametric_jac is ignored)
            return np.ascontiguousarray(self.device_means(X, [params], jac_theta=True)[1][0, i])
        if self.parametric_jac is not None:
            J = np.empty((n, T))
            for j in range(n):
                Jj = np.asarray(self.parametric_jac(X[:, j], th), float)
                if Jj.shape != (self.y_dim, T):
                    raise ValueError(f"parametric_jac must return a {self.y_dim}×{T} matrix, got shape {Jj.shape}")
                J[j] = Jj[i]
            return J
        J = np.empty((n, T))
        for t in range(T):
            h = 1e-6 * max(1.0, abs(th[t]))
            up, dn = th.copy(), th.copy()
            up[t] += h
            dn[t] -= h
            for j in range(n):
                J[j, t] = (float(np.asarray(self.parametric(X[:, j], up))[i]) - float(np.asarray(self.parametric(X[:, j], dn))[i])) / (up[t] - dn[t])
        return J

    # ------------------------------------------------------------------ priors (host bookkeeping)
    def params_sampler(self):
        """_params_sampler (gaussian_process.jl:291-298)."""
        def sample(rng):
            lam = np.stack([np.atleast_1d(p.rand(rng)) for p in self.lengthscale_priors], axis=1)
            amp = np.array([p.rand(rng) for p in self.amplitude_priors])
            sig = np.array([p.rand(rng) for p in self.noise_std_priors])
            th = None if self.theta_priors is None else np.array([p.rand(rng) for p in self.theta_priors])
            return HipGPParams(lam, amp, sig, th)
        return sample

    def params_loglike(self):
        """params_loglike (gaussian_process.jl:282-289)."""
        def ll(p: HipGPParams):
            v = sum(pr.logpdf(p.lengthscales[:, i]) for i, pr in enumerate(self.lengthscale_priors))
            v += sum(pr.logpdf(p.amplitudes[i]) for i, pr in enumerate(self.amplitude_priors))
            v += sum(pr.logpdf(p.noise_std[i]) for i, pr in enumerate(self.noise_std_priors))
            if self.theta_priors is not None:
                v += sum(pr.logpdf(p.theta[i]) for i, pr in enumerate(self.theta_priors))
            return v
        return ll

    # ------------------------------------------------------------------ likelihood
    def data_loglike(self, data: ExperimentData):
        """data_loglike (gaussian_process.jl:250-267): Σ over outputs of logpdf(FiniteGP_i, Y[i,:]).
        Keeps one resident handle per output; each call is one boss_gp_update."""
        gps = [self._new_gp(data.X, data.Y[i]) for i in range(data.Y.shape[0])]

        def ll(p: HipGPParams):
            tot = 0.0
            means = self.mean_values_all(data.X, p)
            for i, g in enumerate(gps):
                try:
                    tot += g.update(p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i], None if means is None else means[i])
                except api.PosDefException:
                    return -math.inf                    # safe_data_loglike (src/surrogate_model.jl:2-12)
            return tot
        ll.handles = gps
        return ll

    def data_loglike_batch(self, data: ExperimentData, samples: Sequence[HipGPParams]) -> np.ndarray:
        """`loglike.(samples)` (src/model_fitters/sampling.jl:64,77) in one batched call per output."""
        S = len(samples)
        tot = np.zeros(S)
        dev = None                                           # DeviceMean: every output's S×N mean rows from one device call
        if device_mean_of(self) is not None and S:
            dev = self.device_means(data.X, samples, api.MEAN_OUTPUT_MAJOR)[0]
        dk = device_kernel_of(self)                          # a program kernel: boss_kgp_loglike_batch, same arrays
        if dk is not None and S == 0:
            return tot
        for i in range(data.Y.shape[0]):
            lam = np.stack([s.lengthscales[:, i] for s in samples], axis=1)
            amp = np.array([s.amplitudes[i] for s in samples])
            sig = np.array([s.noise_std[i] for s in samples])
            means = None
            if dev is not None:
                means = dev[i]
            elif self.parametric is not None:
                means = np.stack([self.mean_values(data.X, s, i) for s in samples], axis=0)
            else:
                mv = self.mean_values(data.X, None, i)
                means = mv
            if dk is not None:
                ll, _ = api.kgp_loglike_batch(data.X, data.Y[i], dk.program, lam, amp, sig, means, self.discrete, self.device)
            else:
                ll, _ = api.loglike_batch(data.X, data.Y[i], self.kernel, lam, amp, sig, means, self.discrete, self.device)
            tot += ll
        return tot

    def _program_loglike_grad(self, data, plist, i, dev, T, tot, gl, ga, gs, gt):
        """Output i of data_loglike_grad_batch under a DeviceKernel(grad=True), added into the caller's arrays."""
        d = plist[0].lengthscales.shape[0]
        # a program kernel (grad=True): the batched calls are built-in-kernel only — per set one update and one
        # loglike_grad[_mean] on ONE resident handle per output, the pattern of data_loglike_batch
        g = self._new_gp(data.X, data.Y[i])
        try:
            for k, p in enumerate(plist):
                if dev is not None:
                    m, J = np.ascontiguousarray(dev[0][i][k]), (dev[1][i][k] if T else None)
                else:
                    m = self.mean_values(data.X, p if self.parametric is not None else None, i)
                    J = self.mean_jacobians(data.X, p, i) if T else None
                try:
                    g.update(p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i], m)
                    if T:
                        ll, gr, dmean = g.loglike_grad_mean()
                        gt[k] += np.asarray(J, float).T @ dmean
                    else:
                        ll, gr = g.loglike_grad()
                except api.PosDefException:
                    tot[k] = -math.inf                   # safe_data_loglike (src/surrogate_model.jl:2-12)
                    continue
                except api.BossError as e:               # an invalid parameter set: -inf, as its status is in the batched calls
                    if e.code != api.BOSS_E_INVALID:
                        raise
                    tot[k] = -math.inf
                    continue
                tot[k] += ll
                gl[k, :, i], ga[k, i], gs[k, i] = gr[:d], gr[d], gr[d + 1]
        finally:
            g.close()

    def data_loglike_grad_batch(self, data: ExperimentData, plist: Sequence[HipGPParams]):
        """data_loglike of every parameter set of `plist` and its gradient w.r.t. (λ, α, σ) AND θ — what ForwardDiff yields
        through data_loglike inside OptimizationMAP (src/model_fitters/optimization.jl:146-164) for a Semiparametric model.
        One device call per output (boss_gp_loglike_grad_batch_mean): every set's own θ gives its mean row and its Jacobian
        J_i (N×T), the device returns J_iᵀ a_i with a_i = K_i⁻¹(y_i − m_i); θ is shared by the outputs, so ∂/∂θ = Σ_i J_iᵀ a_i.
        Returns (ll[S], grads): grads[k] a HipGPParams of gradients (theta None without a parametric mean); a set that fails
        in any output has ll = -inf and zero gradients."""
        refuse_device_kernel(self, "data_loglike_grad_batch (the likelihood gradient of HipGradientMAP)", grad_ok=True)
        S = len(plist)
        tot = np.zeros(S)
        if S == 0:
            return tot, []
        d, P = plist[0].lengthscales.shape
        T = 0 if self.parametric is None else np.asarray(plist[0].theta, float).reshape(-1).shape[0]
        gl, ga, gs, gt = np.zeros((S, d, P)), np.zeros((S, P)), np.zeros((S, P)), np.zeros((S, T))
        dev = None                                           # DeviceMean: means and θ-Jacobians of all sets and outputs from one device call
        if device_mean_of(self) is not None:
            dev = self.device_means(data.X, plist, api.MEAN_OUTPUT_MAJOR, jac_theta=T > 0)
        for i in range(P):
            if device_kernel_of(self) is not None:
                self._program_loglike_grad(data, plist, i, dev, T, tot, gl, ga, gs, gt)
                continue
            lam = np.stack([p.lengthscales[:, i] for p in plist], axis=1)
            amp = np.array([p.amplitudes[i] for p in plist])
            sig = np.array([p.noise_std[i] for p in plist])
            if dev is not None:
                means, jac = dev[0][i], (dev[1][i] if T else None)
            elif self.parametric is not None:
                means = np.stack([self.mean_values(data.X, p, i) for p in plist], axis=0)
                jac = np.stack([self.mean_jacobians(data.X, p, i) for p in plist], axis=0) if T else None
            else:
                means, jac = self.mean_values(data.X, None, i), None
            ll, st, gr, _, dth = api.loglike_grad_batch_mean(data.X, data.Y[i], self.kernel, lam, amp, sig, means, jac, self.discrete,
                                                             self.device)
            tot += np.where(st == 0, ll, -np.inf)
            gl[:, :, i], ga[:, i], gs[:, i] = gr[:d].T, gr[d], gr[d + 1]
            if dth is not None:
                gt += dth.T
        bad = ~np.isfinite(tot)
        tot[bad] = -np.inf
        gl[bad], ga[bad], gs[bad], gt[bad] = 0.0, 0.0, 0.0, 0.0
        return tot, [HipGPParams(gl[k], ga[k], gs[k], gt[k] if self.parametric is not None else None) for k in range(S)]

    # ------------------------------------------------------------------ posterior
    def model_posterior_slice(self, params: HipGPParams, data: ExperimentData, i: int,
                              reserve: int = 0, mean_X=None) -> "HipGaussianProcessPosteriorSlice":
        """model_posterior_slice (gaussian_process.jl:133-141).  reserve: room for later appends.  mean_X: the prior mean of output i
        at data.X where the caller has it already (model_posterior evaluates a DeviceMean once for all outputs)."""
        mX = self.mean_values(data.X, params, i) if mean_X is None else mean_X
        if device_kernel_of(self) is not None:
            if reserve:
                refuse_device_kernel(self, "model_posterior with room for appends (HipSequentialBatchAM)", seq_ok=True)
            g = self._new_gp(data.X, data.Y[i])
            try:
                if reserve:
                    g.reserve(g.N + reserve)
                g.update(params.lengthscales[:, i], params.amplitudes[i], params.noise_std[i], mX)
            except Exception:
                g.close()
                raise
            return HipGaussianProcessPosteriorSlice(self, params, i, g)
        g = api.fit(data.X, data.Y[i], self.kernel, params.lengthscales[:, i], params.amplitudes[i], params.noise_std[i],
                    mX, self.discrete, self.device, reserve)
        return HipGaussianProcessPosteriorSlice(self, params, i, g)

    def model_posterior(self, params, data: ExperimentData, reserve: int = 0):
        """model_posterior (src/posterior.jl:8-19,38-41): a vector of params broadcasts (BI samples)."""
        if isinstance(params, (list, tuple)):
            if len(params) > 1 and reserve == 0:
                # the S samples of a BI fit: per output ONE batched factorisation (boss_gp_fit_batch; boss_kgp_fit_batch under a
                # DeviceKernel) — X and y uploaded once,
                # the S posteriors resident as members of one set.  A sample whose matrix is not positive definite raises, as
                # the reference's cholesky would inside the broadcast (src/posterior.jl:15-19)
                P, S = data.Y.shape[0], len(params)
                dk = device_kernel_of(self)
                per_out = []
                dev = None                                   # DeviceMean: the S×N mean rows of every output from one device call
                if device_mean_of(self) is not None:
                    dev = self.device_means(data.X, params, api.MEAN_OUTPUT_MAJOR)[0]
                for i in range(P):
                    means = [self.mean_values(data.X, p, i) for p in params] if dev is None else list(dev[i])
                    mX = None if all(m is None for m in means) else np.stack([np.zeros(data.X.shape[1]) if m is None else np.asarray(m, float)
                                                                              for m in means])
                    lam = np.stack([p.lengthscales[:, i] for p in params], axis=1)
                    amp, sig = [p.amplitudes[i] for p in params], [p.noise_std[i] for p in params]
                    if dk is not None:
                        gps, _, st = api.kgp_fit_batch(data.X, data.Y[i], dk.program, lam, amp, sig, mX, self.discrete, self.device, grad=dk.grad,
                                                       sequential=dk.sequential)
                    else:
                        gps, _, st = api.fit_batch(data.X, data.Y[i], self.kernel, lam, amp, sig, mX, self.discrete, self.device)
                    if np.any(st != 0):
                        for g in gps:
                            g.close()
                        for row in per_out:
                            for g in row:
                                g.close()
                        bad = int(np.flatnonzero(st)[0])
                        if st[bad] == api.BOSS_E_NOT_PD:
                            raise api.PosDefException(api.BOSS_E_NOT_PD, f"sample {bad}, output {i}: matrix is not positive definite")
                        raise api.BossError(int(st[bad]), f"sample {bad}, output {i}: invalid hyper-parameters")
                    per_out.append(gps)
                return [HipGaussianProcessPosterior([HipGaussianProcessPosteriorSlice(self, params[s], i, per_out[i][s]) for i in range(P)])
                        for s in range(S)]
            return [self.model_posterior(p, data, reserve) for p in params]
        if device_mean_of(self) is not None:                 # one evaluation for all outputs
            mX = self.mean_values_all(data.X, params)
            return HipGaussianProcessPosterior([self.model_posterior_slice(params, data, i, reserve, np.ascontiguousarray(mX[i]))
                                                for i in range(data.Y.shape[0])])
        return HipGaussianProcessPosterior([self.model_posterior_slice(params, data, i, reserve)
                                            for i in range(data.Y.shape[0])])


def _clip(var):
    """_clip_var is applied device-side by boss_gp_predict; nothing to do on the host."""
    return var


@dataclass
class HipGaussianProcessPosteriorSlice:
    """GaussianProcessPosterior (gaussian_process.jl:127-131): one output dimension."""
    model: HipGaussianProcess
    params: HipGPParams
    idx: int
    gp: api.GP

    def _mean_s(self, X):
        return self.model.mean_values(X, self.params, self.idx)

    def mean_and_var(self, x):
        x = np.asarray(x, float)
        if x.ndim == 1:                      # vector -> scalars (gaussian_process.jl:169-173)
            mu, var = self.gp.predict(x[:, None], self._mean_s(x))
            return float(mu[0]), float(var[0])
        return self.gp.predict(x, self._mean_s(x))       # matrix -> vectors (:174-178)

    def mean(self, x):
        return self.mean_and_var(x)[0]

    def var(self, x):
        return self.mean_and_var(x)[1]

    def std(self, x):
        return np.sqrt(self.var(x))

    def mean_and_std(self, x):
        mu, var = self.mean_and_var(x)
        return mu, np.sqrt(var)

    def mean_and_var_grad(self, X, mean_grad=None):
        """mean_and_var(post, X) with its gradient w.r.t. the columns of X (analytic, on the device):
        (mu[M], var[M], dmu[d,M], dvar[d,M]).  mean_grad: d×M gradient of the prior mean, if it has one."""
        refuse_device_kernel(self.model, "mean_and_var_grad", grad_ok=True)
        X = np.asarray(X, float)
        if X.ndim == 1:
            X = X[:, None]
        return self.gp.predict_grad(X, self._mean_s(X), mean_grad)

    def mean_and_cov(self, X):
        """mean_and_cov(post, X::Matrix) (gaussian_process.jl:180-184) -> (mu[M], Σ[M,M])."""
        refuse_device_kernel(self.model, "cov / mean_and_cov")
        X = np.asarray(X, float)
        return self.gp.predict_cov(X, self._mean_s(X))

    def cov(self, X):
        return self.mean_and_cov(X)[1]

    def append(self, x, y_i: float) -> float:
        """Posterior of the data augmented by (x, y_i) under the same hyper-parameters — what
        model_posterior returns after augment_dataset! (problem.jl:191-198) — as a block Cholesky
        append on the resident factor (boss_gp_append).  x: length-d vector or d×n matrix."""
        refuse_device_kernel(self.model, "append", seq_ok=True)
        x = np.asarray(x, float)
        return self.gp.append(x, y_i, self._mean_s(x))

    def close(self):
        self.gp.close()


@dataclass
class HipGaussianProcessPosterior:
    """DefaultModelPosterior (src/posterior.jl:31-79): fan-out over output slices; rows = outputs."""
    slices: List[HipGaussianProcessPosteriorSlice]

    def mean_and_var(self, x):
        res = [s.mean_and_var(x) for s in self.slices]
        x = np.asarray(x, float)
        if x.ndim == 1:
            return np.array([r[0] for r in res]), np.array([r[1] for r in res])
        return np.vstack([r[0] for r in res]), np.vstack([r[1] for r in res])

    def mean(self, x):
        return self.mean_and_var(x)[0]

    def var(self, x):
        return self.mean_and_var(x)[1]

    def std(self, x):
        return np.sqrt(self.var(x))

    def mean_and_std(self, x):
        mu, var = self.mean_and_var(x)
        return mu, np.sqrt(var)

    def mean_and_var_grad(self, X, mean_grad=None):
        """Every slice's mean_and_var_grad stacked: (mu, var [P, M], dmu, dvar [P, d, M]).  mean_grad: None or P×d×M."""
        res = [s.mean_and_var_grad(X, None if mean_grad is None else mean_grad[i]) for i, s in enumerate(self.slices)]
        return tuple(np.stack([r[q] for r in res]) for q in range(4))

    def mean_and_cov(self, X):
        """src/posterior.jl:74-79: means stacked as rows, covariances along dims=3 (M×M×P)."""
        res = [s.mean_and_cov(X) for s in self.slices]
        return np.vstack([r[0] for r in res]), np.stack([r[1] for r in res], axis=2)

    def cov(self, X):
        return self.mean_and_cov(X)[1]

    def append(self, x, y):
        """Append one observation (x, y[P]) (or n of them: x d×n, y P×n) to every output slice."""
        y = np.asarray(y, float)
        for i, s in enumerate(self.slices):
            s.append(x, y[i])

    def close(self):
        for s in self.slices:
            s.close()


def average_mean(posts: Sequence[HipGaussianProcessPosterior], X):
    """average_mean (src/posterior.jl:177-179)."""
    return sum(p.mean(X) for p in posts) / len(posts)
