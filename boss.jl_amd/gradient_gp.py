"""HipGradientGaussianProcess — host-side mirror of the reference's GradientGaussianProcess
(src/models/gradient_gp.jl) and GradientData (src/data/gradient_data.jl) over the C ABI.

Every evaluated point contributes its value and its gradient, so n points give an n(1+x_dim) system per output:
  model_posterior_slice / data_loglike   -> boss_ggp_create + boss_ggp_update (augmented Gram, Cholesky, α-solve, logpdf)
  mean / var / mean_and_var              -> boss_gp_predict on the augmented factor
  mean_and_cov / cov                     -> boss_ggp_predict_cov
  data_loglike_batch (`loglike.(samples)`) -> boss_ggp_loglike_batch (all samples of an output in one call)
  data_loglike_grad_batch (a round of OptimizationMAP) -> boss_ggp_loglike_grad_batch (values and gradients, one call per output)
  augment_dataset! at fixed parameters   -> boss_ggp_append (block rows of the factor, on the device), boss_ggp_reserve
  SequentialBatchAM on fixed candidates  -> gradient_sequential_batch (boss_ggp_track_create + boss_acq_ei_tracks)
The acquisition maximizers (HipBatchAM, …) take these posteriors unchanged.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import api
from .kernel import refuse_device_kernel
from .model import HipGaussianProcessPosterior, HipGaussianProcessPosteriorSlice
from .problem import ExperimentData


@dataclass
class GradientData(ExperimentData):
    """GradientData(X, Y, dY) (gradient_data.jl:25-38): dY is y_dim × x_dim × n, dY[i, k, j] = ∂y_i/∂x_k at X[:, j]."""
    dY: np.ndarray = None

    def __post_init__(self):
        super().__post_init__()
        self.dY = np.asarray(self.dY, float)
        if self.dY.ndim == 2:                                   # a single output given as x_dim × n
            self.dY = self.dY[None, :, :]
        assert self.dY.shape == (self.Y.shape[0], self.X.shape[0], self.X.shape[1]), "dY must be y_dim × x_dim × n"

    def augment(self, x, y, J) -> "GradientData":
        """augment_dataset (gradient_data.jl:47-68): J is the y_dim × x_dim Jacobian at x."""
        x = np.asarray(x, float).reshape(-1, 1)
        y = np.asarray(y, float).reshape(-1, 1)
        J = np.asarray(J, float).reshape(self.Y.shape[0], self.X.shape[0], 1)
        return GradientData(np.hstack([self.X, x]), np.hstack([self.Y, y]), np.concatenate([self.dY, J], axis=2))

    def slice(self, i: int) -> "GradientData":
        """slice(::GradientData, idx) (gradient_data.jl:76-82)."""
        return GradientData(self.X, self.Y[i:i + 1], self.dY[i:i + 1])


@dataclass
class HipGradientGPParams:
    """GradientGaussianProcessParams(λ, α, σ, σ_∂) (gradient_gp.jl:41-51)."""
    lengthscales: np.ndarray      # d×P
    amplitudes: np.ndarray        # P
    noise_std: np.ndarray         # P
    grad_noise_std: np.ndarray    # P

    def __post_init__(self):
        self.lengthscales = np.atleast_2d(np.asarray(self.lengthscales, float))
        self.amplitudes = np.asarray(self.amplitudes, float).reshape(-1)
        self.noise_std = np.asarray(self.noise_std, float).reshape(-1)
        self.grad_noise_std = np.asarray(self.grad_noise_std, float).reshape(-1)

    def slice(self, i: int) -> "HipGradientGPParams":
        """slice(::GradientGaussianProcessParams, idx) (gradient_gp.jl:94-101)."""
        return HipGradientGPParams(self.lengthscales[:, i:i + 1], self.amplitudes[i:i + 1], self.noise_std[i:i + 1],
                                   self.grad_noise_std[i:i + 1])


def join_gradient_slices(ps: Sequence[HipGradientGPParams]) -> HipGradientGPParams:
    """join_slices (gradient_gp.jl:103-110)."""
    return HipGradientGPParams(np.hstack([p.lengthscales for p in ps]), np.concatenate([p.amplitudes for p in ps]),
                               np.concatenate([p.noise_std for p in ps]), np.concatenate([p.grad_noise_std for p in ps]))


class HipGradientGPPosteriorSlice(HipGaussianProcessPosteriorSlice):
    """GradientGPPosteriorSlice (gradient_gp.jl:57-64): μ = k*·α, σ² = max(0, k(x,x) − ‖L⁻¹k*‖²)  (:334-361).
    mean_and_var_grad is inherited: boss_gp_predict_grad takes these posteriors."""

    def _mean_s(self, X):
        return None                                             # the model's mean is not used (:334-337)

    def mean_and_cov(self, X):
        """cov(post::GradientGPPosteriorSlice, X) with its mean (:368-373, boss_ggp_predict_cov) -> (mu[M], Σ[M,M]): neither
        jittered nor clipped."""
        return self.gp.predict_value_cov(np.asarray(X, float))

    def cov(self, X):
        return self.mean_and_cov(X)[1]

    def append(self, x, y, dy) -> float:
        """augment_dataset! (src/types/problem.jl:191-198) on the fitted slice: new points with values and gradients, hyper-parameters
        unchanged (boss_ggp_append: the new points' rows go to the end of the handle's ordering, the block rows of the factor that
        hold them are updated on the device)."""
        return self.gp.append(x, y, dy)

    def reserve(self, extra_points: int) -> float:
        """Storage for `extra_points` further points, so their appends re-allocate nothing (boss_ggp_reserve), then the update under
        the slice's own parameters that a reserve asks for.  Returns the logpdf."""
        g, p, i = self.gp, self.params, self.idx
        g.reserve(points=g.n + int(extra_points))
        return g.update(p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i], p.grad_noise_std[i])

    def track(self, cand: api.Candidates, Xs=None) -> api.GradTrack:
        """The slice's resident state at the candidates `cand` (api.GradTrack); Xs, the same candidates as an array, is taken for
        symmetry with the other models' slices and not read."""
        return api.GradTrack(self.gp, cand)


# Which way an append goes is decided in the library (boss_ggp_append): block rows where at most four 128-row block rows hold new rows,
# a re-factorisation of the resident data on the device otherwise.  Measured on an MI355X (tools/ggp_append_times.py, one process per
# shape, p50 of 20 single-point appends after a reserve, ms; the rebuild timed on the previous commit's library; DESIGN.md §4.2,
# profiles/ggp_append.jsonl):
#   rows   block rows | re-factorisation on the device | the previous commit's rebuild     track extension | prediction
#   1017   0.247      | 0.340                          | 1.341                             0.085           | 0.215
#   4095   0.648      | 1.307                          | 3.151                             0.224           | 0.923
#   9216   1.405      | 7.671                          | 9.628                             0.483           | 3.856
#   1024 (d = 3)  0.230 | 0.332                        | 1.528                             0.050           | 0.206
# The block-row path is the fastest at every measured shape, so no shape is routed to the re-factorisation by a measured boundary.
def gradient_sequential_batch(posts: Sequence[Sequence[HipGradientGPPosteriorSlice]], Xs, batch_size: int, fit_coefs, y_max=None, Y=None,
                              valid_mask=None) -> np.ndarray:
    """SequentialBatchAM (src/acquisition_maximizers/batch.jl:26-38) over the fixed candidates Xs d×M for the S sampled
    gradient-observation posteriors posts[s][i]: `batch_size` times the arg-max of EI × feasibility is selected by one
    boss_acq_ei_tracks call, a speculative observation is appended to every slice, and the acquisition is re-evaluated on the
    extended tracks.

    The reference's own SequentialBatchAM cannot run on GradientData: speculative_evaluation! calls augment_dataset!(problem, x, y)
    without a Jacobian (batch.jl:32-37), while augment_dataset(::GradientData, x, results::Tuple) unpacks two elements
    (gradient_data.jl:47-53).  The extension chosen here: the speculative observation is (x, ŷ, ∇ŷ) with ŷ the sample-averaged
    posterior mean μ(x) and ∇ŷ the sample-averaged ∇μ(x) (mean_and_var_grad) — the posterior mean of a derivative observation is
    the derivative of the posterior mean.

    Storage for `batch_size` further points is reserved up front (slice.reserve: one re-update per slice under its own parameters;
    a member of a fitted set leaves the set there), so every append is a block-row update that re-allocates nothing and a track's
    capacity is never exceeded.  Y (P×N, the observations so far; None: no best-so-far yet) gives EI's incumbent through
    best_so_far and grows with the speculative values.  Returns the d×batch_size selections."""
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
        for row in posts:
            for p in row:
                p.reserve(batch_size)
        for row in posts:                                       # (one by one: whatever was created is closed on an exception)
            tracks.append([])
            for p in row:
                tracks[-1].append(p.track(cand, Xs))
        xs = []
        for _ in range(batch_size):
            b = None if Yrun is None else best_so_far(LinFitness(coefs), Yrun, ymax)
            _, am, _ = api.acq_ei_tracks(tracks, coefs, y_max, b, valid_mask, want_acq=False)
            x = Xs[:, am].copy()
            y, dy = np.zeros(P), np.zeros((P, Xs.shape[0]))
            for row in posts:
                for i, p in enumerate(row):
                    mu, _, dmu, _ = p.mean_and_var_grad(x[:, None])
                    y[i] += float(np.asarray(mu).reshape(-1)[0]) / S
                    dy[i] += np.asarray(dmu, float).reshape(-1) / S
            for row in posts:
                for i, p in enumerate(row):
                    p.append(x, y[i], dy[i])
            Yrun = y[:, None] if Yrun is None else np.concatenate([Yrun, y[:, None]], axis=1)
            xs.append(x)
        return np.stack(xs, axis=1)
    finally:
        for ts in tracks:
            for t in ts:
                t.close()
        cand.close()


# Where data_loglike_batch switches from the loop of boss_ggp_update calls on one resident handle to one boss_ggp_loglike_batch
# call.  Measured on an MI355X (tools/model_batch_time.py, p50 of 20 calls, range of three runs, ms; DESIGN.md §4.2,
# profiles/model_batch_times.jsonl):
#   rows   S = 2: batched | loop        S = 8: batched | loop        S = 64: batched | loop
#     60   0.117-0.121 | 0.229-0.230    0.115-0.119 | 0.932-0.942    0.120-0.122 | 7.37-7.51
#   1017   0.382-0.402 | 0.567-0.591    0.462-0.478 | 2.27-2.36      1.22-1.24   | 17.4-18.8
#   4095   2.12-2.17   | 2.24-2.26      4.87-4.97   | 8.96-9.06      32.0        | 71.9-72.4
#   8190   8.94-9.02   | 9.13-9.17      29.2-29.4   | 36.5-36.6      225-226     | 293
# The batched call wins at every measured shape, by less and less as the system grows (the resident chain of a single update is
# at its best there); beyond 8190 rows nothing is measured and the loop stays.  One set is an update.
BATCH_MIN_SETS = 2
BATCH_MAX_ROWS = 8192


def batched_call_pays(rows: int, n_sets: int) -> bool:
    """True where one batched call scores `n_sets` parameter sets of an augmented system of `rows` = n(1+d) rows faster than
    the loop on resident handles (the measured region above)."""
    return n_sets >= BATCH_MIN_SETS and rows <= BATCH_MAX_ROWS


# Where data_loglike_grad_batch switches from the loop of boss_ggp_update + boss_ggp_loglike_grad on one resident handle to one
# boss_ggp_loglike_grad_batch call.  Measured on an MI355X (tools/model_llgrad_batch_time.py, one process per shape, p50 of 20 calls,
# range of three runs, ms; the loop timed on the previous commit's library; DESIGN.md §4.2, profiles/model_llgrad_batch_times.jsonl):
#   rows   S = 8: batched | loop          S = 64: batched | loop
#     60   0.334-0.346 | 2.15-2.28        0.438-0.454 | 17.1-19.0
#    240   0.340-0.365 | 2.30-2.37        0.497-0.543 | 18.3-19.0
#   1017   1.15-1.18   | 6.00-6.07        3.91-4.18   | 47.8-52.2
#   2043   3.15-3.21   | 11.1-11.3        19.0-19.2   | 88.8-93.5
#   4095   18.9-19.3   | 24.5-25.0        124-125     | 196-199
# The batched call's slowest run is below the loop's fastest at every measured shape (1.27× at the least, at 4095 rows and 8 sets).
# Fewer than 8 sets and more than 4095 rows are not measured: they keep the loop.
GRAD_BATCH_MIN_SETS = 8
GRAD_BATCH_MAX_ROWS = 4095


def batched_grad_call_pays(rows: int, n_sets: int) -> bool:
    """True where one batched call evaluates value and gradient of `n_sets` parameter sets of an augmented system of `rows` =
    n(1+d) rows faster than the loop on a resident handle: the measured region above, where the batched call's slowest run stays
    below the loop's fastest.  Unmeasured shapes keep the loop."""
    return n_sets >= GRAD_BATCH_MIN_SETS and rows <= GRAD_BATCH_MAX_ROWS


@dataclass
class HipGradientGaussianProcess:
    """GradientGaussianProcess(mean, kernel, lengthscale_priors, amplitude_priors, noise_std_priors,
    grad_noise_std_priors) (gradient_gp.jl:22-31).  `mean` is carried like the reference does and, like there,
    used by neither the posterior nor the likelihood."""
    lengthscale_priors: Sequence
    amplitude_priors: Sequence
    noise_std_priors: Sequence
    grad_noise_std_priors: Sequence
    mean: object = None
    kernel: str = "matern52"
    device: int = 0

    sliceable = True                                            # gradient_gp.jl:69

    def __post_init__(self):
        refuse_device_kernel(self, "HipGradientGaussianProcess (the augmented Gram matrix needs the kernel's derivatives)")

    @property
    def y_dim(self):
        return len(self.amplitude_priors)

    def params_sampler(self):
        def sample(rng):
            lam = np.stack([np.atleast_1d(p.rand(rng)) for p in self.lengthscale_priors], axis=1)
            return HipGradientGPParams(lam, np.array([p.rand(rng) for p in self.amplitude_priors]),
                                       np.array([p.rand(rng) for p in self.noise_std_priors]),
                                       np.array([p.rand(rng) for p in self.grad_noise_std_priors]))
        return sample

    def params_loglike(self):
        """params_loglike (gradient_gp.jl:403-411)."""
        def ll(p: HipGradientGPParams):
            v = sum(pr.logpdf(p.lengthscales[:, i]) for i, pr in enumerate(self.lengthscale_priors))
            v += sum(pr.logpdf(p.amplitudes[i]) for i, pr in enumerate(self.amplitude_priors))
            v += sum(pr.logpdf(p.noise_std[i]) for i, pr in enumerate(self.noise_std_priors))
            v += sum(pr.logpdf(p.grad_noise_std[i]) for i, pr in enumerate(self.grad_noise_std_priors))
            return v
        return ll

    def data_loglike(self, data: GradientData):
        """data_loglike (gradient_gp.jl:367-397), summed over the outputs; one resident handle per output,
        each call one boss_ggp_update.  A non-PD augmented matrix yields -Inf (safe_data_loglike)."""
        gps = [api.GradGP(data.X, data.Y[i], data.dY[i], self.kernel, self.device) for i in range(data.Y.shape[0])]

        def ll(p: HipGradientGPParams):
            tot = 0.0
            for i, g in enumerate(gps):
                try:
                    tot += g.update(p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i], p.grad_noise_std[i])
                except api.PosDefException:
                    return -math.inf
            return tot
        ll.handles = gps
        return ll

    def data_loglike_grad(self, data: GradientData):
        """data_loglike with its gradient w.r.t. (λ, α, σ, σ_∂) — what ForwardDiff yields through gradient_gp.jl:367-397 inside
        OptimizationMAP (src/model_fitters/optimization.jl:146-164): p -> (ℓ, HipGradientGPParams of partial derivatives), per
        output one boss_ggp_update + boss_ggp_loglike_grad on a resident handle.  Non-PD: (-Inf, zeros)."""
        gps = [api.GradGP(data.X, data.Y[i], data.dY[i], self.kernel, self.device) for i in range(data.Y.shape[0])]

        def llg(p: HipGradientGPParams):
            d, P = p.lengthscales.shape
            gl, ga, gs, gd = np.zeros((d, P)), np.zeros(P), np.zeros(P), np.zeros(P)
            tot = 0.0
            for i, g in enumerate(gps):
                try:
                    g.update(p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i], p.grad_noise_std[i])
                except api.PosDefException:
                    return -math.inf, HipGradientGPParams(np.zeros((d, P)), np.zeros(P), np.zeros(P), np.zeros(P))
                ll, gr = g.loglike_grad()
                tot += ll
                gl[:, i], ga[i], gs[i], gd[i] = gr[:d], gr[d], gr[d + 1], gr[d + 2]
            return tot, HipGradientGPParams(gl, ga, gs, gd)
        llg.handles = gps
        return llg

    def data_loglike_batch(self, data: GradientData, samples: Sequence[HipGradientGPParams]) -> np.ndarray:
        """`loglike.(samples)` (src/model_fitters/sampling.jl:64,77) — what HipBatchedMAP and HipSampleOptMAP's scoring phase call:
        one boss_ggp_loglike_batch call per output (every launch covers all samples), summed over the outputs, -Inf where any
        output's augmented matrix is not PD.  Few samples of a large system stay a loop of boss_ggp_update calls on resident
        handles (`batched_call_pays`)."""
        samples = list(samples)
        S = len(samples)
        if S == 0:
            return np.zeros(0)
        d, n = data.X.shape
        if not batched_call_pays(n * (1 + d), S):
            ll = self.data_loglike(data)
            try:
                return np.array([ll(p) for p in samples])
            finally:
                for g in ll.handles:
                    g.close()
        tot = np.zeros(S)
        for i in range(data.Y.shape[0]):
            lam = np.stack([p.lengthscales[:, i] for p in samples], axis=1)
            amp, sig, sgd = (np.array([getattr(p, name)[i] for p in samples]) for name in ("amplitudes", "noise_std", "grad_noise_std"))
            ll_i, st = api.ggp_loglike_batch(data.X, data.Y[i], data.dY[i], self.kernel, lam, amp, sig, sgd, self.device)
            tot += np.where(st == api.BOSS_OK, ll_i, -math.inf)
        return tot

    def data_loglike_grad_batch(self, data: GradientData, samples: Sequence[HipGradientGPParams]):
        """Value and gradient of data_loglike at every parameter set of `samples` — one round of a multistart OptimizationMAP
        (src/model_fitters/optimization.jl:146-164): (ℓ[S], [HipGradientGPParams of partial derivatives] × S), summed over the
        outputs, by ONE boss_ggp_loglike_grad_batch call per output; (-Inf, zeros) where any output's augmented matrix is not PD.
        Where the batched call does not pay (`batched_grad_call_pays`) the sets go through data_loglike_grad's loop on resident
        handles; both ways give the same numbers bit for bit."""
        samples = list(samples)
        S = len(samples)
        if S == 0:
            return np.zeros(0), []
        d, n = data.X.shape
        P = data.Y.shape[0]
        if not batched_grad_call_pays(n * (1 + d), S):
            llg = self.data_loglike_grad(data)
            try:
                res = [llg(p) for p in samples]
            finally:
                for g in llg.handles:
                    g.close()
            return np.array([r[0] for r in res]), [r[1] for r in res]
        tot = np.zeros(S)
        gl, ga, gs, gd = np.zeros((S, d, P)), np.zeros((S, P)), np.zeros((S, P)), np.zeros((S, P))
        for i in range(P):
            lam = np.stack([p.lengthscales[:, i] for p in samples], axis=1)
            amp, sig, sgd = (np.array([getattr(p, name)[i] for p in samples]) for name in ("amplitudes", "noise_std", "grad_noise_std"))
            ll_i, st, gr = api.ggp_loglike_grad_batch(data.X, data.Y[i], data.dY[i], self.kernel, lam, amp, sig, sgd, self.device)
            tot += np.where(st == api.BOSS_OK, ll_i, -math.inf)
            gl[:, :, i], ga[:, i], gs[:, i], gd[:, i] = gr[:d].T, gr[d], gr[d + 1], gr[d + 2]
        bad = ~np.isfinite(tot)
        tot[bad] = -math.inf
        for arr in (gl, ga, gs, gd):
            arr[bad] = 0.0
        return tot, [HipGradientGPParams(gl[k], ga[k], gs[k], gd[k]) for k in range(S)]

    def model_posterior_slice(self, params: HipGradientGPParams, data: GradientData, i: int) -> HipGradientGPPosteriorSlice:
        """model_posterior_slice (gradient_gp.jl:307-329)."""
        g = api.GradGP(data.X, data.Y[i], data.dY[i], self.kernel, self.device)
        try:
            g.update(params.lengthscales[:, i], params.amplitudes[i], params.noise_std[i], params.grad_noise_std[i])
        except Exception:
            g.close()
            raise
        return HipGradientGPPosteriorSlice(self, params, i, g)

    def model_posterior(self, params, data: GradientData):
        if isinstance(params, (list, tuple)):
            return self.model_posterior_batch(list(params), data)
        return HipGaussianProcessPosterior([self.model_posterior_slice(params, data, i) for i in range(data.Y.shape[0])])

    def model_posterior_batch(self, samples: Sequence[HipGradientGPParams], data: GradientData):
        """`model_posterior.(Ref(model), samples, Ref(data))` (src/posterior.jl:15-19): one posterior per sample of a BI fit, built
        by ONE boss_ggp_fit_batch call per output (the members share the points and observations and are predicted together by
        acq_ei).  Few samples of a large system, or a batch that does not fit the device, stay the loop of create + update per sample
        and output (`batched_call_pays`).  A sample whose matrix is not PD raises PosDefException, as the loop does."""
        S = len(samples)
        d, n = data.X.shape

        def loop():
            return [self.model_posterior(p, data) for p in samples]
        if S == 0 or not batched_call_pays(n * (1 + d), S):
            return loop()
        rows = []                                               # rows[i][s]: handle of output i under sample s

        def close_all():
            for gps in rows:
                for g in gps:
                    g.close()
        for i in range(data.Y.shape[0]):
            lam = np.stack([p.lengthscales[:, i] for p in samples], axis=1)
            amp, sig, sgd = (np.array([getattr(p, name)[i] for p in samples]) for name in ("amplitudes", "noise_std", "grad_noise_std"))
            try:
                gps, _, st = api.ggp_fit_batch(data.X, data.Y[i], data.dY[i], self.kernel, lam, amp, sig, sgd, self.device)
            except api.BossError as e:
                close_all()
                if e.code == api.BOSS_E_ALLOC:                  # (a 36 864-row member is 10.9 GB: the loop holds one factor at a time per handle)
                    return loop()
                raise
            rows.append(gps)
            bad = np.flatnonzero(st != api.BOSS_OK)
            if bad.size:
                close_all()
                s = int(bad[0])
                if st[s] == api.BOSS_E_NOT_PD:
                    raise api.PosDefException(api.BOSS_E_NOT_PD, f"sample {s}, output {i}: the augmented matrix is not positive definite")
                raise api.BossError(int(st[s]), f"sample {s}, output {i}: invalid hyper-parameters")
        return [HipGaussianProcessPosterior([HipGradientGPPosteriorSlice(self, p, i, rows[i][s]) for i in range(len(rows))])
                for s, p in enumerate(samples)]
