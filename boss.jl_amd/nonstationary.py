"""HipNonstationaryGP — host-side mirror of the reference's NonstationaryGP posterior
(src/models/nonstationary_gp/nonstationary_gp.jl) over the C ABI.

The reference models the lengthscales / amplitudes / noise stds as functions of the input — posteriors of latent
ParametrizedGPs or constants (`_param_posterior_slice`, :198-212).  Those latent models are host-side closures here
(`f_lam(x) -> x_dim vector`, `f_amp(x) -> scalar`, `f_noise(x) -> scalar`, one triple per output); the dense work —
Gibbs Gram matrix, Cholesky, likelihood, prediction — runs on the device (`boss_ngp_*`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import numpy as np

from . import api
from .kernel import refuse_device_kernel
from .problem import ExperimentData


def _cols(f: Callable, X: np.ndarray) -> np.ndarray:
    """f at every column of X: rows = points.  Closures flagged `vectorized` take the whole d×M matrix at once
    (the ParametrizedGP posteriors below: one device call for all points)."""
    if getattr(f, "vectorized", False):
        return np.asarray(f(X), float)
    return np.array([np.asarray(f(X[:, j]), float) for j in range(X.shape[1])])


# ---------------------------------------------------------------------------------------------
# Activation functions the device knows in closed form (BOSS_ACT_*): ordinary array functions that also carry their code, so that
# a ParametrizedGP using them can be evaluated by the resident latent kernel (HipParametrizedGP.device_spec).
# ---------------------------------------------------------------------------------------------
class LatentActivation:
    def __init__(self, name: str, par: float = 0.0):
        self.name, self.par = name, float(par)

    def __call__(self, z):
        z = np.asarray(z, float)
        if self.name == "softplus":                         # softplus / ScaledSoftplus (src/utils/bijectors.jl:116-158), overflow-safe
            return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z))) + self.par
        if self.name == "exp":
            return np.exp(z)
        return z

    def with_lower_bound(self, lb: float) -> "LatentActivation":
        """ScaledSoftplus(lb): softplus(z) + lb."""
        if self.name != "softplus":
            raise ValueError("only softplus takes a lower bound")
        return LatentActivation("softplus", lb)

    def __repr__(self):
        return f"LatentActivation({self.name!r}, {self.par})"


identity_act = LatentActivation("identity")
softplus = LatentActivation("softplus")
exp_act = LatentActivation("exp")


def latent_transform(spec, m):
    """The closed forms the device evaluates for spec = (target, (p0, p1), activation, par) (HipParametrizedGP.device_spec) at the
    latent posterior means m: returns (value, d value / d m) — quantile(target, cdf(Normal(), m)) |> act and its derivative."""
    from scipy.special import ndtr
    target, (p0, p1), act, par = spec
    m = np.asarray(m, float)
    if target == "normal":
        z, dz = p0 + p1 * m, np.full_like(m, p1)
    elif target == "lognormal":
        z = np.exp(p0 + p1 * m)
        dz = p1 * z
    elif target == "uniform":
        z, dz = p0 + (p1 - p0) * ndtr(m), (p1 - p0) * np.exp(-0.5 * m * m) / math.sqrt(2.0 * math.pi)
    elif target == "none":
        z, dz = m, np.ones_like(m)
    else:
        raise ValueError(f"unknown target {target!r}")
    if act == "softplus":
        e = np.exp(-np.abs(z))
        return np.maximum(z, 0.0) + np.log1p(e) + par, dz * np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    if act == "exp":
        v = np.exp(z)
        return v, dz * v
    if act == "identity":
        return z, dz
    raise ValueError(f"unknown activation {act!r}")


def constant_latent(value: float) -> Callable:
    """A latent model that is a constant (`_param_posterior_slice` of a non-GP parameter, nonstationary_gp.jl:198-212): a vectorized
    closure that also says so (`.constant`), which lets the resident latent kernel take it."""
    value = float(value)

    def post(x):
        x = np.asarray(x, float)
        return value if x.ndim == 1 else np.full(x.shape[1], value)
    post.vectorized = True
    post.constant = value
    return post


# ---------------------------------------------------------------------------------------------
# ParametrizedGP (src/models/nonstationary_gp/parametrized_gp.jl): the latent model of one hyper-parameter
# of the NonstationaryGP — a zero-mean, unit-amplitude GP over the data points whose (whitened) outputs are the
# parameters; its posterior mean, pushed through Normal-cdf -> target quantile -> activation, is the value of
# the hyper-parameter at x.
# ---------------------------------------------------------------------------------------------
@dataclass
class HipParametrizedGPParams:
    """ParametrizedGPParams(X, μ, L, yϵ, λ) (parametrized_gp.jl:64-76)."""
    X: np.ndarray
    mu: np.ndarray
    L: np.ndarray
    yeps: np.ndarray
    lengthscale: np.ndarray


@dataclass
class HipParametrizedGP:
    """ParametrizedGP(kernel, lengthscale_prior, target_dist, act_func, noise_std) (:39-47).  The reference requires a
    Dirac lengthscale prior (:193): `lengthscale` holds its values.  `target_dist`: None or anything with `.ppf(u)`
    (a frozen scipy.stats distribution); `act_func` must accept arrays."""
    lengthscale: Sequence[float]
    kernel: str = "matern32"
    target_dist: object = None
    act_func: Callable = identity_act
    noise_std: float = 0.0
    device: int = 0

    def __post_init__(self):
        refuse_device_kernel(self, "HipNonstationaryGP (a latent HipParametrizedGP; the nonstationary kernel itself is the Gibbs kernel)")

    def transform(self, y):
        """construct_variable_transform (:122-134) then act_func: z = quantile(target, cdf(Normal(0,1), y))."""
        y = np.asarray(y, float)
        if self.target_dist is not None:
            from scipy.special import ndtr
            y = self.target_dist.ppf(ndtr(y))
        return self.act_func(y)

    def device_spec(self):
        """(target, (p0, p1), activation, par) — the names of api.LATENT_TARGETS / api.LATENT_ACTS — when transform() is one of the
        closed forms the device evaluates (include/bosship.h, boss_nlat_create), else None.  Recognised: target_dist None, frozen
        scipy.stats norm, lognorm with loc 0 and uniform; activations identity_act, softplus (optionally with a lower bound), exp_act.
            Normal(μ, σ): z = μ + σ m;  LogNormal(μ, σ) = lognorm(s=σ, scale=e^μ): z = exp(μ + σ m);  Uniform(a, b): z = a + (b − a) Φ(m)
        — what quantile(target, cdf(Normal(), m)) equals."""
        act = self.act_func
        if not isinstance(act, LatentActivation):
            return None
        t = self.target_dist
        if t is None:
            return ("none", (0.0, 0.0), act.name, act.par)
        dist = getattr(t, "dist", None)
        name = getattr(dist, "name", None)
        if name not in ("norm", "lognorm", "uniform"):
            return None
        try:
            shapes, loc, scale = dist._parse_args(*t.args, **t.kwds)
            loc, scale = float(loc), float(scale)
        except Exception:
            return None
        if name == "norm":
            return ("normal", (loc, scale), act.name, act.par)
        if name == "uniform":
            return ("uniform", (loc, loc + scale), act.name, act.par)
        if loc != 0.0 or not scale > 0.0:
            return None
        return ("lognormal", (math.log(scale), float(shapes[0])), act.name, act.par)

    def params_sampler(self, data: ExperimentData):
        """_params_sampler (:191-215): L = chol of the prior covariance at the data points (finite_param_gp, :136-158),
        yϵ ~ N(0, I)."""
        lam = np.asarray(self.lengthscale, float)
        n = data.X.shape[1]
        g = api.GP(data.X, np.zeros(n), self.kernel, None, self.device)
        try:
            g.update(lam, 1.0, self.noise_std)
            L, _ = g.factor()
        finally:
            g.close()
        mu = np.zeros(n)

        def sample(rng):
            return HipParametrizedGPParams(data.X, mu, L, rng.standard_normal(n), lam)
        return sample

    def params_loglike(self, data: ExperimentData = None):
        """params_loglike (:160-189): logpdf(MvNormal(0, I), yϵ)."""
        return lambda p: float(-0.5 * (p.yeps @ p.yeps) - 0.5 * len(p.yeps) * math.log(2.0 * math.pi))

    def model_posterior(self, params: HipParametrizedGPParams, data: ExperimentData = None):
        """model_posterior (:90-106): x -> act(ft(mean of the GP posterior conditioned on y = L yϵ + μ)).  The returned
        closure takes one point or a d×M matrix (one device call); `.close()` releases the handle; `.gp` is its api.GP handle and
        `.model` this model (what a resident latent object is built from)."""
        y = params.L @ params.yeps + params.mu
        g = api.GP(params.X, y, self.kernel, None, self.device)
        g.update(params.lengthscale, 1.0, self.noise_std)

        def post(x):
            x = np.asarray(x, float)
            m, _ = g.predict(x[:, None] if x.ndim == 1 else x)
            z = self.transform(m)
            return float(z[0]) if x.ndim == 1 else z
        post.vectorized = True
        post.close = g.close
        post.gp = g
        post.model = self
        return post

    def model_posterior_lookup(self, params: HipParametrizedGPParams, data: ExperimentData = None):
        """model_posterior_lookup (:108-120): the values at the data points only, no kernel matrix."""
        vals = self.transform(params.L @ params.yeps + params.mu)
        table = {tuple(params.X[:, j]): float(vals[j]) for j in range(params.X.shape[1])}

        def post(x):
            x = np.asarray(x, float)
            if x.ndim == 1:
                return table[tuple(x)]
            return np.array([table[tuple(x[:, j])] for j in range(x.shape[1])])
        post.vectorized = True
        return post


def stack_latents(posts: Sequence[Callable]) -> Callable:
    """x -> apply.(posts, Ref(x)) (nonstationary_gp.jl:209-212): the x_dim latent lengthscale models of one output as
    one closure returning a d-vector (or M×d for a matrix of points)."""
    def f(x):
        x = np.asarray(x, float)
        cols = [np.asarray(p(x), float) for p in posts]
        return np.array(cols) if x.ndim == 1 else np.stack(cols, axis=1)
    f.vectorized = all(getattr(p, "vectorized", False) for p in posts)
    f.posts = list(posts)
    return f


def _latent_arg(post, name: str):
    """What api.NgpLatents takes for one latent closure: a float, or (handle, spec).  ValueError naming the latent otherwise."""
    if hasattr(post, "constant"):
        return float(post.constant)
    model, gp = getattr(post, "model", None), getattr(post, "gp", None)
    if isinstance(model, HipParametrizedGP) and gp is not None:
        spec = model.device_spec()
        if spec is not None:
            return (gp, spec)
        raise ValueError(f"resident_latents: the transform of latent {name} (target_dist {model.target_dist!r}, act_func "
                         f"{model.act_func!r}) is not one the device evaluates")
    raise ValueError(f"resident_latents: latent {name} is neither a constant (constant_latent) nor a HipParametrizedGP posterior")


@dataclass
class HipNonstationaryPosteriorSlice:
    """GaussianProcessPosterior over the NonstationaryKernel (nonstationary_gp.jl:153-157)."""
    gp: api.GibbsGP
    f_lam: Callable
    f_amp: Callable
    mean_fn: Optional[Callable]
    discrete: Optional[np.ndarray]
    f_noise: Optional[Callable] = None                          # σ(·): needed by append only
    latents: Optional[api.NgpLatents] = None                    # the latent models resident on the device (resident_latents)

    def append(self, x, y) -> float:
        """augment_dataset! (src/types/problem.jl:191-198) on the fitted slice: the latent models are evaluated at the new points and
        the block rows of the factor that hold them are rebuilt on the device (boss_ngp_append).  x: d×m (or length d), y: m.
        Returns the logpdf of all points."""
        if self.f_noise is None:
            raise ValueError("this slice was built without its noise model")
        X = np.asarray(x, float).reshape(self.gp.d, -1)
        Xr = self._round(X)
        ms = None if self.mean_fn is None else np.array([float(self.mean_fn(X[:, j])) for j in range(X.shape[1])])
        if self.latents is not None:                            # (the kernel rounds for λ and α, σ sees the point as given)
            lam, amp, noi, _, _ = self.latents.eval(X, jac=False, noise=self.latents.has_noise)
            if noi is None:
                noi = _cols(self.f_noise, X).reshape(-1)
            return self.gp.append(X, np.asarray(y, float).reshape(-1), lam, amp, noi, ms)
        return self.gp.append(X, np.asarray(y, float).reshape(-1), _cols(self.f_lam, Xr).T, _cols(self.f_amp, Xr).reshape(-1),
                              _cols(self.f_noise, X).reshape(-1), ms)

    def track(self, cand: api.Candidates, Xs) -> api.GibbsTrack:
        """The slice's resident predictive state at the candidates `cand` (= api.Candidates of Xs d×M): the latent closures are
        evaluated at the rounded candidates, or the resident latents on the device; `append` then extends it in O(N·M)."""
        Xs = np.asarray(Xs, float)
        ms = None if self.mean_fn is None else np.array([float(self.mean_fn(Xs[:, j])) for j in range(Xs.shape[1])])
        if self.latents is not None:
            return api.GibbsTrack(self.gp, cand, mean_Xs=ms, latents=self.latents)
        Xr = self._round(Xs)
        return api.GibbsTrack(self.gp, cand, _cols(self.f_lam, Xr).T, _cols(self.f_amp, Xr).reshape(-1), ms)

    def loglike_grad(self):
        """(logpdf, dlam[d, N], damp[N], dnoise[N], dmean[N]): data_loglike_slice (nonstationary_gp.jl:237-245) of the fitted slice and
        its partial derivatives w.r.t. the latent models' values at the training points (boss_ngp_loglike_grad) — the cotangents a
        gradient-based fitter chains through its latent models."""
        return self.gp.loglike_grad()

    def _round(self, X):
        if self.discrete is None:
            return X
        X = X.copy()
        X[self.discrete] = np.rint(X[self.discrete])            # DiscreteKernel: the kernel, hence λ(·), α(·), sees rounded inputs
        return X

    def mean_and_var(self, x):
        x = np.asarray(x, float)
        vec = x.ndim == 1
        X = x[:, None] if vec else x
        Xr = self._round(X)
        ms = None if self.mean_fn is None else np.array([float(self.mean_fn(X[:, j])) for j in range(X.shape[1])])
        if self.latents is not None:
            mu, var = self.gp.predict_lat(X, self.latents, ms)
            return (float(mu[0]), float(var[0])) if vec else (mu, var)
        mu, var = self.gp.predict(X, _cols(self.f_lam, Xr).T, _cols(self.f_amp, Xr).reshape(-1), ms)
        return (float(mu[0]), float(var[0])) if vec else (mu, var)

    def mean_and_var_grad(self, X, lam_jac: Optional[Callable] = None, amp_jac: Optional[Callable] = None, mean_grad=None,
                          fd_step: float = 1e-6):
        """mean_and_var and its gradient w.r.t. the candidate columns (boss_ngp_predict_grad) — what ForwardDiff pushes through the
        posterior inside OptimizationAM (src/acquisition_maximizers/optimization.jl:36).  The candidate also enters through the latent
        λ(x*), α(x*): `lam_jac(x) -> d×d` ([l, m] = ∂λ_l/∂x_m) and `amp_jac(x) -> d` supply their Jacobians; without them central
        differences of the host closures are taken (step fd_step).  With resident latents the values and analytic Jacobians are
        evaluated on the device (boss_ngp_predict_grad_lat); lam_jac / amp_jac / fd_step are not used.
        Returns (mu[M], var[M], dmu[d, M], dvar[d, M])."""
        X = np.asarray(X, float)
        if X.ndim == 1:
            X = X[:, None]
        d, M = X.shape
        if self.latents is not None:
            ms = None if self.mean_fn is None else np.array([float(self.mean_fn(X[:, j])) for j in range(M)])
            return self.gp.predict_grad_lat(X, self.latents, ms, mean_grad)
        Xr = self._round(X)

        def jac(f, x, n_out):
            J = np.zeros((n_out, d))
            for m in range(d):
                e = np.zeros(d)
                e[m] = fd_step
                J[:, m] = (np.atleast_1d(np.asarray(f(x + e), float)) - np.atleast_1d(np.asarray(f(x - e), float))) / (2 * fd_step)
            return J
        Dl = np.stack([np.asarray(lam_jac(Xr[:, j]), float) if lam_jac else jac(self.f_lam, Xr[:, j], d) for j in range(M)], axis=2)
        Da = np.stack([np.asarray(amp_jac(Xr[:, j]), float).reshape(-1) if amp_jac else jac(self.f_amp, Xr[:, j], 1)[0] for j in range(M)], axis=1)
        if self.discrete is not None:                        # rounded dimensions: the latent models are piecewise constant in them
            Dl[:, self.discrete, :] = 0.0
            Da[self.discrete, :] = 0.0
        ms = None if self.mean_fn is None else np.array([float(self.mean_fn(X[:, j])) for j in range(M)])
        return self.gp.predict_grad(X, _cols(self.f_lam, Xr).T, _cols(self.f_amp, Xr).reshape(-1), Dl, Da, ms, mean_grad)

    def mean_and_cov(self, X):
        """mean_and_cov(post, X::Matrix) (gaussian_process.jl:180-184) over the Gibbs kernel -> (mu[M], Σ[M,M]) with the diagonal
        through _clip_var (boss_ngp_predict_cov); the latent models are evaluated at the rounded candidates, as in mean_and_var."""
        X = np.asarray(X, float)
        if X.ndim == 1:
            X = X[:, None]
        Xr = self._round(X)
        ms = None if self.mean_fn is None else np.array([float(self.mean_fn(X[:, j])) for j in range(X.shape[1])])
        if self.latents is not None:
            lam, amp, _, _, _ = self.latents.eval(X, jac=False)
            return self.gp.predict_cov(X, lam, amp, ms)
        return self.gp.predict_cov(X, _cols(self.f_lam, Xr).T, _cols(self.f_amp, Xr).reshape(-1), ms)

    def cov(self, X):
        return self.mean_and_cov(X)[1]

    def mean(self, x):
        return self.mean_and_var(x)[0]

    def var(self, x):
        return self.mean_and_var(x)[1]

    def std(self, x):
        return np.sqrt(self.var(x))

    def close(self):
        if self.latents is not None:
            self.latents.close()
        self.gp.close()


@dataclass
class HipNonstationaryGP:
    """finite_nongp (nonstationary_gp.jl:183-196) for y_dim outputs: per output i the closures
    f_lam[i], f_amp[i], f_noise[i] and an optional prior mean function."""
    f_lam: Sequence[Callable]
    f_amp: Sequence[Callable]
    f_noise: Sequence[Callable]
    mean: Optional[Sequence[Optional[Callable]]] = None
    discrete: Optional[Sequence[bool]] = None
    device: int = 0
    # keep every output's latent models resident on the device (api.NgpLatents): the slices evaluate λ(x*), α(x*) and their
    # analytic Jacobians there instead of through the host closures.  Needs f_lam[i] = stack_latents(...) of constants
    # (constant_latent) and HipParametrizedGP posteriors whose transform device_spec() describes, f_amp[i] one of them; ValueError else.
    resident_latents: bool = False

    def __post_init__(self):
        if self.resident_latents:
            for i in range(len(self.f_lam)):
                self._latent_args(i)

    def _latent_args(self, i):
        posts = getattr(self.f_lam[i], "posts", None)
        if posts is None:
            raise ValueError(f"resident_latents: f_lam[{i}] must be built by stack_latents from its per-dimension latent models")
        lam = [_latent_arg(p, f"f_lam[{i}][{l}]") for l, p in enumerate(posts)]
        amp = _latent_arg(self.f_amp[i], f"f_amp[{i}]")
        try:                                                    # σ(·) is optional on the device: append falls back to its closure
            noise = _latent_arg(self.f_noise[i], f"f_noise[{i}]")
        except ValueError:
            noise = None
        return lam, amp, noise

    def _slice_latents(self, i) -> Optional[api.NgpLatents]:
        if not self.resident_latents:
            return None
        lam, amp, noise = self._latent_args(i)
        return api.NgpLatents(lam, amp, noise, self.discrete, self.device)

    def _latent_at_data(self, X, i):
        disc = None if self.discrete is None else np.asarray(self.discrete, bool)
        Xr = X.copy()
        if disc is not None:
            Xr[disc] = np.rint(Xr[disc])
        m = None if self.mean is None or self.mean[i] is None else np.array([float(self.mean[i](X[:, j])) for j in range(X.shape[1])])
        return _cols(self.f_lam[i], Xr).T, _cols(self.f_amp[i], Xr).reshape(-1), _cols(self.f_noise[i], X).reshape(-1), m, disc

    def model_posterior_slice(self, data: ExperimentData, i: int) -> HipNonstationaryPosteriorSlice:
        lam, amp, noi, m, disc = self._latent_at_data(data.X, i)
        g = api.GibbsGP(data.X, data.Y[i], disc, self.device)
        try:
            g.update(lam, amp, noi, m)
            lat = self._slice_latents(i)
        except Exception:
            g.close()
            raise
        return HipNonstationaryPosteriorSlice(g, self.f_lam[i], self.f_amp[i], None if self.mean is None else self.mean[i], disc, self.f_noise[i],
                                              lat)

    def model_posterior(self, data: ExperimentData) -> List[HipNonstationaryPosteriorSlice]:
        return [self.model_posterior_slice(data, i) for i in range(data.Y.shape[0])]

    def data_loglike(self, data: ExperimentData) -> float:
        """data_loglike (nonstationary_gp.jl:231-245): Σ over outputs of logpdf(FiniteGP_i, Y[i, :]); -Inf when not PD."""
        tot = 0.0
        for i in range(data.Y.shape[0]):
            lam, amp, noi, m, disc = self._latent_at_data(data.X, i)
            g = api.GibbsGP(data.X, data.Y[i], disc, self.device)
            try:
                tot += g.update(lam, amp, noi, m)
            except api.PosDefException:
                return -np.inf
            finally:
                g.close()
        return tot


def data_loglike_batch(models: Sequence[HipNonstationaryGP], data: ExperimentData) -> np.ndarray:
    """`loglike.(samples)` (src/model_fitters/sampling.jl:59-78) for S nonstationary models that differ in their latent closures
    only (same `discrete`, same `device`): every model's closures are evaluated at the data exactly as `data_loglike` evaluates them
    (λ, α at the rounded points, σ and the prior mean at the points as given), then ONE boss_ngp_loglike_batch call per output
    scores all of them.  Returns the S log-likelihoods summed over the outputs; -Inf where an output's matrix is not PD (or a
    latent value is invalid)."""
    models = list(models)
    S = len(models)
    if S == 0:
        return np.zeros(0)
    first, disc0 = _check_batch_models(models)
    d, N = data.X.shape
    tot = np.zeros(S)
    for i in range(data.Y.shape[0]):
        lam = np.empty((d, N, S), order="F")
        amp = np.empty((N, S), order="F")
        noi = np.empty((N, S), order="F")
        means = []
        for s, m in enumerate(models):
            lam[:, :, s], amp[:, s], noi[:, s], mu, _ = m._latent_at_data(data.X, i)
            means.append(mu)
        mean_X = None if all(mu is None for mu in means) else np.stack([np.zeros(N) if mu is None else mu for mu in means])
        ll, st = api.ngp_loglike_batch(data.X, data.Y[i], lam, amp, noi, mean_X, disc0, first.device)
        tot += np.where(st == api.BOSS_OK, ll, -np.inf)
    return tot


def data_loglike_grad_batch(models: Sequence[HipNonstationaryGP], data: ExperimentData):
    """data_loglike_batch with the cotangents a gradient-based fitter chains back through its latent models: for S nonstationary
    models that differ in their latent closures only (same `discrete`, same `device`) the closures are evaluated at the data as
    `_latent_at_data` evaluates them (λ, α at the rounded points, σ and the prior mean at the points as given), then ONE
    boss_ngp_loglike_grad_batch call per output gives every model's log-likelihood and its partial derivatives w.r.t. those values.
    Returns (ℓ[S] summed over the outputs, grads) with grads[s][i] = (dlam[d, N], damp[N], dnoise[N], dmean[N]) of model s and
    output i — what HipNonstationaryPosteriorSlice.loglike_grad returns for that slice; -Inf and zeros throughout a model's
    cotangents where one of its outputs is not PD (or holds an invalid latent value)."""
    models = list(models)
    S = len(models)
    if S == 0:
        return np.zeros(0), []
    first, disc0 = _check_batch_models(models)
    d, N = data.X.shape
    P = data.Y.shape[0]
    tot = np.zeros(S)
    grads = [[None] * P for _ in range(S)]
    for i in range(P):
        lam = np.empty((d, N, S), order="F")
        amp = np.empty((N, S), order="F")
        noi = np.empty((N, S), order="F")
        means = []
        for s, m in enumerate(models):
            lam[:, :, s], amp[:, s], noi[:, s], mu, _ = m._latent_at_data(data.X, i)
            means.append(mu)
        mean_X = None if all(mu is None for mu in means) else np.stack([np.zeros(N) if mu is None else mu for mu in means])
        ll, st, dlam, damp, dnoise, dmean = api.ngp_loglike_grad_batch(data.X, data.Y[i], lam, amp, noi, mean_X, disc0, first.device)
        tot += np.where(st == api.BOSS_OK, ll, -np.inf)
        for s in range(S):
            grads[s][i] = (np.array(dlam[:, :, s]), np.array(damp[:, s]), np.array(dnoise[:, s]), np.array(dmean[:, s]))
    for s in np.flatnonzero(~np.isfinite(tot)):
        tot[s] = -np.inf
        grads[s] = [tuple(np.zeros_like(a) for a in g) for g in grads[s]]
    return tot, grads


def _check_batch_models(models):
    first = models[0]
    disc0 = None if first.discrete is None else np.asarray(first.discrete, bool)
    for m in models[1:]:
        disc = None if m.discrete is None else np.asarray(m.discrete, bool)
        if m.device != first.device or (disc is None) != (disc0 is None) or (disc is not None and not np.array_equal(disc, disc0)):
            raise ValueError("the models of a batch must share `discrete` and `device`")
    return first, disc0


def nonstationary_model_posterior_batch(models: Sequence[HipNonstationaryGP], data: ExperimentData) -> List[List[HipNonstationaryPosteriorSlice]]:
    """`model_posterior.(samples, Ref(data))` (src/posterior.jl:15-19) for S nonstationary models that differ in their latent closures
    only (same `discrete`, same `device`): the closures are evaluated at the data as `model_posterior_slice` evaluates them, then ONE
    boss_ngp_fit_batch call per output builds the S posteriors as resident handles that share the points and observations.  Returns
    posts[s][i] (sample s, output i).  A sample whose matrix is not PD raises PosDefException, as `model_posterior` does."""
    models = list(models)
    S = len(models)
    if S == 0:
        return []
    first, disc0 = _check_batch_models(models)
    d, N = data.X.shape
    rows = []
    for i in range(data.Y.shape[0]):
        lam = np.empty((d, N, S), order="F")
        amp = np.empty((N, S), order="F")
        noi = np.empty((N, S), order="F")
        means = []
        for s, m in enumerate(models):
            lam[:, :, s], amp[:, s], noi[:, s], mu, _ = m._latent_at_data(data.X, i)
            means.append(mu)
        mean_X = None if all(mu is None for mu in means) else np.stack([np.zeros(N) if mu is None else mu for mu in means])
        try:
            gps, _, st = api.ngp_fit_batch(data.X, data.Y[i], lam, amp, noi, mean_X, disc0, first.device)
        except Exception:
            for r in rows:
                for g in r:
                    g.close()
            raise
        rows.append(gps)
        bad = np.flatnonzero(st != api.BOSS_OK)
        if bad.size:
            for r in rows:
                for g in r:
                    g.close()
            s = int(bad[0])
            if st[s] == api.BOSS_E_NOT_PD:
                raise api.PosDefException(api.BOSS_E_NOT_PD, f"sample {s}, output {i}: the matrix is not positive definite")
            raise api.BossError(int(st[s]), f"sample {s}, output {i}: invalid latent values")
    lats = []
    try:
        for m in models:
            for i in range(len(rows)):
                lats.append(m._slice_latents(i))
    except Exception:                                       # e.g. a latent handle closed since its model was built: nothing is left behind
        for lat in lats:
            if lat is not None:
                lat.close()
        for r in rows:
            for g in r:
                g.close()
        raise
    P = len(rows)
    return [[HipNonstationaryPosteriorSlice(rows[i][s], m.f_lam[i], m.f_amp[i], None if m.mean is None else m.mean[i], disc0, m.f_noise[i],
                                            lats[i + P * s])
             for i in range(P)] for s, m in enumerate(models)]


def nonstationary_acq_ei_batch(posts: Sequence[Sequence[HipNonstationaryPosteriorSlice]], Xs, fit_coefs, y_max=None, best=None,
                               valid_mask=None):
    """EI × feasibility averaged over the S sampled posteriors posts[s][i] (src/acquisitions/expected_improvement.jl:87-90) at the
    candidates Xs d×M: per output ONE boss_ngp_predict_set call (every sample's latent models evaluated at the rounded candidates,
    all samples in one prediction launch where they come from nonstationary_model_posterior_batch), then boss_acq_ei_moments.
    Returns (acq[M], argmax, max)."""
    Xs = np.asarray(Xs, float)
    if Xs.ndim == 1:
        Xs = Xs[:, None]
    S, P = len(posts), len(posts[0])
    d, M = Xs.shape
    mu = np.empty((S, P, M))
    var = np.empty((S, P, M))
    resident = all(p.latents is not None for row in posts for p in row)      # latent values read on the device (the _lat set call)
    for i in range(P):
        sl = [posts[s][i] for s in range(S)]
        if resident:
            means = [None if p.mean_fn is None else np.array([float(p.mean_fn(Xs[:, j])) for j in range(M)]) for p in sl]
            ms = None if all(m is None for m in means) else np.stack([np.zeros(M) if m is None else m for m in means])
            mu[:, i, :], var[:, i, :] = api.ngp_predict_set_lat([p.gp for p in sl], Xs, [p.latents for p in sl], ms)
            continue
        Xr = sl[0]._round(Xs)
        lam = np.empty((d, M, S), order="F")
        amp = np.empty((M, S), order="F")
        means = []
        for s, p in enumerate(sl):
            lam[:, :, s] = _cols(p.f_lam, Xr).T
            amp[:, s] = _cols(p.f_amp, Xr).reshape(-1)
            means.append(None if p.mean_fn is None else np.array([float(p.mean_fn(Xs[:, j])) for j in range(M)]))
        ms = None if all(m is None for m in means) else np.stack([np.zeros(M) if m is None else m for m in means])
        mu[:, i, :], var[:, i, :] = api.ngp_predict_set([p.gp for p in sl], Xs, lam, amp, ms)
    return api.acq_ei_moments(mu, var, fit_coefs, y_max, best, valid_mask, posts[0][0].gp.device)


def nonstationary_sequential_batch(posts: Sequence[Sequence[HipNonstationaryPosteriorSlice]], Xs, batch_size: int, fit_coefs, y_max=None,
                                   Y=None, valid_mask=None) -> np.ndarray:
    """SequentialBatchAM (src/acquisition_maximizers/batch.jl:26-38) over the fixed candidates Xs d×M for the S sampled nonstationary
    posteriors posts[s][i] (nonstationary_model_posterior_batch, or [model.model_posterior(data)]): `batch_size` times the arg-max of
    EI × feasibility is selected, the speculative observation (x, ŷ = the sample-averaged posterior mean, average_mean) is appended
    to every slice, and the acquisition is re-evaluated.  Every slice's candidate state stays resident (slice.track): a selection
    costs one boss_acq_ei_tracks call, an O(N²) block-row append per slice and an O(N·M) extension of its track.  Y (P×N, the
    observations so far; None: no best-so-far yet) gives EI's incumbent through best_so_far and grows with the speculative
    observations.  Members of a fitted set leave the set on their first append; storage grows where an append crosses a 256-row
    boundary (nothing is reserved up front: a reserve would need the latent values at the data again, which the slices do not
    keep).  Returns the d×batch_size selections."""
    from .problem import LinFitness, best_so_far
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    posts = [list(row) for row in posts]
    if not posts or not posts[0]:
        raise ValueError("posts must hold at least one sample with at least one output")
    Xs = np.asarray(Xs, float)
    if Xs.ndim == 1:
        Xs = Xs[:, None]
    S, P = len(posts), len(posts[0])
    coefs = np.asarray(fit_coefs, float).reshape(-1)
    ymax = np.full(P, np.inf) if y_max is None else np.asarray(y_max, float).reshape(-1)
    Yrun = None if Y is None else np.asarray(Y, float).reshape(P, -1)
    dev = posts[0][0].gp.device
    cand = api.Candidates(Xs, dev)
    tracks = []
    try:
        tracks = [[p.track(cand, Xs) for p in row] for row in posts]
        xs = []
        for _ in range(batch_size):
            b = None if Yrun is None else best_so_far(LinFitness(coefs), Yrun, ymax)
            _, am, _ = api.acq_ei_tracks(tracks, coefs, y_max, b, valid_mask, want_acq=False)
            x = Xs[:, am].copy()
            y = sum(np.array([t.moments(am, 1)[0][0] for t in ts]) for ts in tracks) / S       # ŷ read off the tracks: average_mean
            for row in posts:
                for i, p in enumerate(row):
                    p.append(x, y[i])
            Yrun = y[:, None] if Yrun is None else np.concatenate([Yrun, y[:, None]], axis=1)
            xs.append(x)
        return np.stack(xs, axis=1)
    finally:
        for ts in tracks:
            for t in ts:
                t.close()
        cand.close()


def nonstationary_acq_ei_grad_batch(posts: Sequence[Sequence[HipNonstationaryPosteriorSlice]], Xs, fit_coefs, y_max=None, best=None,
                                    valid_mask=None, lam_jac=None, amp_jac=None, mean_grad=None, fd_step: float = 1e-6):
    """EI × feasibility AND its gradient w.r.t. the candidates, averaged over the S sampled posteriors posts[s][i]
    (src/acquisitions/expected_improvement.jl:87-90 under the ForwardDiff of OptimizationAM, optimization.jl:89-118) at the candidates
    Xs d×M in ONE boss_ngp_acq_ei_grad_set call.  Every slice's latent closures are evaluated at the rounded candidates; their
    Jacobians come from lam_jac[s][i](x) -> d×d / amp_jac[s][i](x) -> d, or by central differences of the closures (step fd_step),
    exactly as HipNonstationaryPosteriorSlice.mean_and_var_grad takes them; discrete dimensions get zero columns.  mean_grad: None or
    [S][P][d][M].  Returns (acq[M], dacq[d, M])."""
    Xs = np.asarray(Xs, float)
    if Xs.ndim == 1:
        Xs = Xs[:, None]
    S, P = len(posts), len(posts[0])
    if any(len(row) != P for row in posts):
        raise ValueError("posts must be S rows of P slices")
    d, M = Xs.shape
    n = S * P
    if all(p.latents is not None for row in posts for p in row):
        # resident latent models: values and analytic Jacobians are evaluated on the device (lam_jac / amp_jac / fd_step are not used)
        means = [None if p.mean_fn is None else np.array([float(p.mean_fn(Xs[:, j])) for j in range(M)]) for row in posts for p in row]
        ms = None if all(m is None for m in means) else np.stack([np.zeros(M) if m is None else m for m in means])
        mg = None if mean_grad is None else np.asarray(mean_grad, float).reshape(n, d, M)
        return api.ngp_acq_ei_grad_set_lat([[p.gp for p in row] for row in posts], Xs, [[p.latents for p in row] for row in posts],
                                           fit_coefs, y_max, best, valid_mask, ms, mg)
    Xr = posts[0][0]._round(Xs)
    lam = np.empty((d, M, n), order="F")
    amp = np.empty((M, n), order="F")
    Dl = np.empty((d, d, M, n), order="F")
    Da = np.empty((d, M, n), order="F")
    means = []

    def jac(f, x, n_out):
        J = np.zeros((n_out, d))
        for m in range(d):
            e = np.zeros(d)
            e[m] = fd_step
            J[:, m] = (np.atleast_1d(np.asarray(f(x + e), float)) - np.atleast_1d(np.asarray(f(x - e), float))) / (2 * fd_step)
        return J
    for s in range(S):
        for i in range(P):
            p, k = posts[s][i], i + P * s
            lj = None if lam_jac is None else lam_jac[s][i]
            aj = None if amp_jac is None else amp_jac[s][i]
            lam[:, :, k] = _cols(p.f_lam, Xr).T
            amp[:, k] = _cols(p.f_amp, Xr).reshape(-1)
            for j in range(M):
                Dl[:, :, j, k] = np.asarray(lj(Xr[:, j]), float) if lj else jac(p.f_lam, Xr[:, j], d)
                Da[:, j, k] = np.asarray(aj(Xr[:, j]), float).reshape(-1) if aj else jac(p.f_amp, Xr[:, j], 1)[0]
            means.append(None if p.mean_fn is None else np.array([float(p.mean_fn(Xs[:, j])) for j in range(M)]))
    disc = posts[0][0].discrete
    if disc is not None:                                     # rounded dimensions: the latent models are piecewise constant in them
        Dl[:, disc, :, :] = 0.0
        Da[disc, :, :] = 0.0
    ms = None if all(m is None for m in means) else np.stack([np.zeros(M) if m is None else m for m in means])
    mg = None if mean_grad is None else np.asarray(mean_grad, float).reshape(n, d, M)
    return api.ngp_acq_ei_grad_set([[p.gp for p in row] for row in posts], Xs, lam, amp, Dl, Da, fit_coefs, y_max, best, valid_mask, ms, mg)


# ---------------------------------------------------------------------------------------------
# HipNonstationaryModel — the reference's NonstationaryGP STRUCT (nonstationary_gp.jl:60-110) with latent MODELS in place of the
# closures of HipNonstationaryGP: what a model fitter moves are the whitened outputs yϵ of the latent ParametrizedGPs (and the scalar
# parameters of distribution latents); the data log-likelihood and its gradient w.r.t. those run on the device (api.NgpWhitened).
# ---------------------------------------------------------------------------------------------
@dataclass
class HipNonstationaryParams:
    """NonstationaryGPParams(λ, α, σ) (nonstationary_gp.jl:112-130): per output i the d lengthscale latents lam[i][l], the amplitude
    latent amp[i] and the noise latent noise[i]; each a HipParametrizedGPParams or a float (a distribution latent's value)."""
    lam: List[List[object]]
    amp: List[object]
    noise: List[object]

    def latents(self, i):
        return list(self.lam[i]) + [self.amp[i], self.noise[i]]


@dataclass
class HipNonstationaryModel:
    """Per output i: lengthscale_models[i][l] (l < d), amplitude_models[i], noise_std_models[i] — each a HipParametrizedGP whose
    transform device_spec() describes, or a univariate prior of problem.py (Dirac, LogNormal: the latent is that one number at every
    point, `_param_posterior_slice` of a UnivariateDistribution, nonstationary_gp.jl:200-203)."""
    lengthscale_models: Sequence[Sequence[object]]
    amplitude_models: Sequence[object]
    noise_std_models: Sequence[object]
    mean: Optional[Sequence[Optional[Callable]]] = None
    discrete: Optional[Sequence[bool]] = None
    device: int = 0
    resident_latents: bool = False                              # of the HipNonstationaryGP model_posterior builds

    def __post_init__(self):
        self._handles = {}
        for i in range(self.y_dim):
            for q, m in enumerate(self._models(i)):
                if isinstance(m, HipParametrizedGP) and m.device_spec() is None:
                    raise ValueError(f"resident_latents: the transform of latent {self._name(i, q)} (target_dist {m.target_dist!r}, "
                                     f"act_func {m.act_func!r}) is not one the device evaluates")

    @property
    def y_dim(self):
        return len(self.amplitude_models)

    def _models(self, i):
        return list(self.lengthscale_models[i]) + [self.amplitude_models[i], self.noise_std_models[i]]

    def _name(self, i, q):
        d = len(self.lengthscale_models[i])
        return f"lengthscale_models[{i}][{q}]" if q < d else ("amplitude_models", "noise_std_models")[q - d] + f"[{i}]"

    # ---- priors
    def params_sampler(self, data: ExperimentData):
        """_params_sampler (nonstationary_gp.jl:281-300): every ParametrizedGP latent through HipParametrizedGP.params_sampler (L, μ;
        latents with the same kernel, lengthscales and noise share one factor), every distribution latent through rand."""
        shared = {}

        def one(m):
            if not isinstance(m, HipParametrizedGP):
                return lambda rng: float(m.rand(rng))
            key = (m.kernel, tuple(np.asarray(m.lengthscale, float)), float(m.noise_std), m.device)
            if key not in shared:
                shared[key] = m.params_sampler(data)
            return shared[key]
        samplers = [[one(m) for m in self._models(i)] for i in range(self.y_dim)]

        def sample(rng):
            vals = [[s(rng) for s in row] for row in samplers]
            return HipNonstationaryParams([v[:-2] for v in vals], [v[-2] for v in vals], [v[-1] for v in vals])
        return sample

    def params_loglike(self, data: ExperimentData = None):
        """params_loglike (nonstationary_gp.jl:250-279): Σ over the latents — logpdf(MvNormal(0, I), yϵ) or the prior's logpdf."""
        def ll(p: HipNonstationaryParams):
            tot = 0.0
            for i in range(self.y_dim):
                for m, v in zip(self._models(i), p.latents(i)):
                    tot += m.params_loglike(data)(v) if isinstance(m, HipParametrizedGP) else float(m.logpdf(v))
            return tot
        return ll

    # ---- the flat parameter vector
    def _layout(self, data: ExperimentData):
        """[(i, q, start, length)] in the order of vectorizer (nonstationary_gp.jl:302-330): all λ latents (output after output),
        then all α, then all σ."""
        N = data.X.shape[1]
        d = data.X.shape[0]
        order = [(i, q) for i in range(self.y_dim) for q in range(d)] + [(i, d) for i in range(self.y_dim)] + \
                [(i, d + 1) for i in range(self.y_dim)]
        out, at = [], 0
        for i, q in order:
            n = N if isinstance(self._models(i)[q], HipParametrizedGP) else 1
            out.append((i, q, at, n))
            at += n
        return out, at

    def vectorizer(self, data: ExperimentData):
        """(vectorize(params) -> vector, devectorize(params, vector) -> params): yϵ of the ParametrizedGP latents and the values of
        the distribution latents (Dirac-fixed ones included: a fitter leaves them where they are)."""
        layout, T = self._layout(data)

        def vectorize(p: HipNonstationaryParams):
            v = np.zeros(T)
            for i, q, at, n in layout:
                x = p.latents(i)[q]
                v[at:at + n] = x.yeps if isinstance(x, HipParametrizedGPParams) else float(x)
            return v

        def devectorize(p: HipNonstationaryParams, v):
            v = np.asarray(v, float)
            rows = [p.latents(i) for i in range(self.y_dim)]
            for i, q, at, n in layout:
                x = rows[i][q]
                rows[i][q] = HipParametrizedGPParams(x.X, x.mu, x.L, v[at:at + n].copy(), x.lengthscale) \
                    if isinstance(x, HipParametrizedGPParams) else float(v[at])
            return HipNonstationaryParams([r[:-2] for r in rows], [r[-2] for r in rows], [r[-1] for r in rows])
        return vectorize, devectorize

    # ---- the data term on the device
    def _handle(self, data: ExperimentData, template: HipNonstationaryParams, i: int) -> api.NgpWhitened:
        """The resident whitening of output i (api.NgpWhitened), built from the template's L and μ and kept while the same data
        and factors come back (a fit asks for it once per round)."""
        lat = template.latents(i)
        gps = [x for x in lat if isinstance(x, HipParametrizedGPParams)]
        ent = self._handles.get(i)
        if ent is not None and ent[0] is data.X and ent[1] is data.Y and len(ent[2]) == len(gps) and \
                all(a.L is b.L and a.mu is b.mu for a, b in zip(ent[2], gps)):
            return ent[3]
        if ent is not None:
            ent[3].close()
        N = data.X.shape[1]
        factors, factor_of, specs = [], [], []
        mu = np.zeros((N, len(lat)), order="F")
        for q, (m, x) in enumerate(zip(self._models(i), lat)):
            if not isinstance(x, HipParametrizedGPParams):
                factor_of.append(-1)
                specs.append(None)
                continue
            f = next((k for k, L in enumerate(factors) if L is x.L), None)
            if f is None:
                factors.append(x.L)
                f = len(factors) - 1
            factor_of.append(f)
            specs.append(m.device_spec())
            mu[:, q] = x.mu
        mean = None if self.mean is None or self.mean[i] is None else np.array([float(self.mean[i](data.X[:, j])) for j in range(N)])
        h = api.NgpWhitened(data.X, data.Y[i], factors, factor_of, specs, mu, mean, self.discrete, self.device)
        self._handles[i] = (data.X, data.Y, gps, h)
        return h

    def _theta_rows(self, data, i):
        layout, _ = self._layout(data)
        d = data.X.shape[0]
        by_q = {q: (at, n) for ii, q, at, n in layout if ii == i}
        return np.concatenate([np.arange(by_q[q][0], by_q[q][0] + by_q[q][1]) for q in range(d + 2)])

    def data_loglike_grad_vec(self, data: ExperimentData, template: HipNonstationaryParams, Theta, want_grad: bool = True):
        """The data log-likelihood (summed over the outputs) of every column of Theta (vectorizer layout, T×S) and its gradient
        w.r.t. Theta: ONE boss_nfit_loglike_grad call per output for all columns.  L, μ come from `template`.  Returns (ℓ[S],
        grad[T, S] or None); -Inf and a zero column where a set is invalid or not PD in any output."""
        Theta = np.asarray(Theta, float)
        if Theta.ndim == 1:
            Theta = Theta[:, None]
        S = Theta.shape[1]
        tot = np.zeros(S)
        G = np.zeros(Theta.shape) if want_grad else None
        for i in range(self.y_dim):
            rows = self._theta_rows(data, i)
            ll, st, gr = self._handle(data, template, i).loglike_grad(Theta[rows, :], want_grad)
            tot += np.where(st == api.BOSS_OK, ll, -np.inf)
            if want_grad:
                G[rows, :] = gr
        bad = ~np.isfinite(tot)
        tot[bad] = -np.inf
        if want_grad:
            G[:, bad] = 0.0
        return tot, G

    def data_loglike_grad_batch(self, data: ExperimentData, params_list: Sequence[HipNonstationaryParams]):
        """data_loglike (nonstationary_gp.jl:234-248) of S parameter sets that share L and μ (the draws of one params_sampler, the
        iterates of a fit) and its gradient in the vectorizer's layout: (ℓ[S], grad[T, S])."""
        params_list = list(params_list)
        if not params_list:
            return np.zeros(0), np.zeros((self._layout(data)[1], 0))
        vec, _ = self.vectorizer(data)
        return self.data_loglike_grad_vec(data, params_list[0], np.stack([vec(p) for p in params_list], axis=1))

    def data_loglike_batch(self, data: ExperimentData, params_list: Sequence[HipNonstationaryParams]) -> np.ndarray:
        params_list = list(params_list)
        if not params_list:
            return np.zeros(0)
        vec, _ = self.vectorizer(data)
        return self.data_loglike_grad_vec(data, params_list[0], np.stack([vec(p) for p in params_list], axis=1), want_grad=False)[0]

    # ---- the fitted model
    def posterior_model(self, params: HipNonstationaryParams, data: ExperimentData) -> HipNonstationaryGP:
        """The HipNonstationaryGP whose closures are the latents' posteriors (`_param_posterior_slice`, nonstationary_gp.jl:200-214)."""
        def post(m, x):
            return m.model_posterior(x, data) if isinstance(m, HipParametrizedGP) else constant_latent(float(x))
        f_lam, f_amp, f_noise = [], [], []
        for i in range(self.y_dim):
            posts = [post(m, x) for m, x in zip(self._models(i), params.latents(i))]
            f_lam.append(stack_latents(posts[:-2]))
            f_amp.append(posts[-2])
            f_noise.append(posts[-1])
        return HipNonstationaryGP(f_lam, f_amp, f_noise, self.mean, self.discrete, self.device, self.resident_latents)

    def model_posterior(self, params: HipNonstationaryParams, data: ExperimentData) -> List[HipNonstationaryPosteriorSlice]:
        """model_posterior (nonstationary_gp.jl:140-157): the slices of the fitted model — prediction, resident latents, append and
        tracks work on them as on any HipNonstationaryGP's."""
        return self.posterior_model(params, data).model_posterior(data)

    def close(self):
        for ent in self._handles.values():
            ent[3].close()
        self._handles = {}
