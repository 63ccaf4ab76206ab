"""HipBatchAM — the AcquisitionMaximizer of the plugin trio.

Reproduces SamplingAM (src/acquisition_maximizers/sampling.jl:20-75: draw M candidates from
x_prior inside the domain, acq on each, arg-max) and GridAM (grid.jl:52-65: a fixed list of
points) with ONE device call for all candidates: posterior mean/variance for every output and
hyper-parameter sample, analytic EI × feasibility, make_safe mask, arg-max
(construct_acquisition(::ExpectedImprovement), src/acquisitions/expected_improvement.jl:49-90).

Multi-GPU (one process per GPU), selected by `shard`:
  "candidates"  every rank holds the (redundantly factorised) posterior and evaluates its
                contiguous shard of the candidates; the per-rank (max, global index) pairs are
                combined with a single 16-byte all-gather over RCCL;
  "outputs"     output i is factorised and predicted on rank i mod G only; the (mu_i, var_i) rows
                are all-gathered and the EI x feasibility epilogue + arg-max run from those moments;
  "samples"     hyper-parameter sample s (BI) is factorised on its shard's rank only; the partial
                sums of acq_s(x_j) are combined with one all-reduce(sum) of M doubles.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np

from . import acquisition as acq_host
from . import api
from . import distributed as dist_util
from .acq_program import DeviceAcquisition
from .fitness import DeviceFitness
from .kernel import device_kernel_of, refuse_device_kernel
from .mean import device_mean_of
from .model import HipGaussianProcessPosterior
from .problem import BossOptions, BossProblem, NonlinFitness, best_so_far, in_bounds, in_cons, in_domain
from .transformed import HipTransformedModel, HipTransformedPosterior, warped_acquisition_values, warped_value_and_grad


def _unwarped(posts):
    """Posteriors of a HipTransformedModel without transforms are the base model's: (posts to go on with, whether they are warped)."""
    if not posts or not isinstance(posts[0], HipTransformedPosterior):
        return posts, False
    if posts[0]._identity():
        return [p.base for p in posts], False
    return posts, True


def _no_warp(problem: BossProblem, what: str):
    if isinstance(problem.model, HipTransformedModel):
        raise NotImplementedError(f"{what} is not supported for a HipTransformedModel (use shard='candidates' on a single device)")


def _program_acquisition(problem: BossProblem, what: str = "") -> bool:
    """Whether the problem's acquisition is a DeviceAcquisition (asked before anything reads `.fitness`); `what`: a mode that does
    not take one."""
    if not isinstance(getattr(problem, "acquisition", None), DeviceAcquisition):
        return False
    if what:
        raise NotImplementedError(f"{what} is not supported for a DeviceAcquisition (the traced acquisition program runs on a single "
                                  "device: use shard='candidates', 'outputs' or 'samples' without devices=[...])")
    if isinstance(problem.model, HipTransformedModel):
        raise NotImplementedError("a DeviceAcquisition is not supported for a HipTransformedModel (the program's moments would be "
                                  "model-space moments)")
    return True


def _program_mask(problem: BossProblem, Xs):
    if not problem.acquisition.cons_safe:
        return None
    return in_bounds(Xs, problem.domain.bounds) & in_cons(Xs, problem.domain.cons)


def _rand_in_domain(x_prior: Callable, domain, rng, max_attempts: int):
    """_rand_in_domain / _rand_in_discrete (sampling.jl:59-75)."""
    for _ in range(max_attempts):
        x = np.asarray(x_prior(rng), float)
        x = np.where(domain.discrete, np.rint(x), x)
        if in_domain(x, domain)[0]:
            return x
    return None


def posteriors_of(problem: BossProblem, lo: Optional[int] = None, hi: Optional[int] = None, reserve: int = 0):
    """model_posterior(problem) (src/posterior.jl:2-3): list over BI samples of posteriors.
    [lo, hi) restricts the construction to a shard of the samples; reserve: room for later appends."""
    params = problem.params
    if lo is not None:
        params = (list(params) if isinstance(params, (list, tuple)) else [params])[lo:hi]   # (a MAP fit is one sample)
        if not params:
            return []
    post = problem.model.model_posterior(params, problem.data, reserve) if reserve else \
        problem.model.model_posterior(params, problem.data)
    return post if isinstance(post, list) else [post]


def n_samples(problem: BossProblem) -> int:
    return len(problem.params) if isinstance(problem.params, (list, tuple)) else 1


def output_moments(problem: BossProblem, i: int, Xs: np.ndarray) -> np.ndarray:
    """(mu_i, var_i) of output i at all candidates for every hyper-parameter sample: [S][2][M].
    Only the owner rank of output i factorises it (model_posterior_slice, gaussian_process.jl:133-141)."""
    plist = list(problem.params) if isinstance(problem.params, (list, tuple)) else [problem.params]
    out = np.empty((len(plist), 2, Xs.shape[1]))
    for s, prm in enumerate(plist):
        sl = problem.model.model_posterior_slice(prm, problem.data, i)
        out[s, 0], out[s, 1] = sl.mean_and_var(Xs)
        sl.gp.close()
    return out


def moments_acquisition(problem: BossProblem, mu: np.ndarray, var: np.ndarray, Xs: np.ndarray, q=None):
    """EI x feasibility + arg-max on the device from gathered moments mu/var [S][P][M].  q: a DeviceAcquisition's runtime scalars of
    this maximisation (default: asked for here)."""
    ei = problem.acquisition
    if _program_acquisition(problem):
        q = ei.scalars(problem) if q is None else q
        return api.acq_prog_moments(mu, var, ei.program, q, _program_mask(problem, Xs), ei.outside, problem.model.device)
    b = best_so_far(ei.fitness, problem.data.Y, problem.y_max)
    mask = None
    if ei.cons_safe:
        mask = in_bounds(Xs, problem.domain.bounds) & in_cons(Xs, problem.domain.cons)
    return api.acq_ei_moments(mu, var, ei.fitness.coefs, problem.y_max, b, mask, problem.model.device)


def _device_mean_model(posts):
    """The model of the posteriors when its prior mean is a DeviceMean (one boss_mean_eval serves all samples and outputs), else None."""
    model = getattr(posts[0].slices[0], "model", None)
    return model if device_mean_of(model) is not None else None


def _device_prior_means(posts, Xs, jac_x: bool = False):
    """(S×P×M prior means, S×P×d×M ∂m/∂x or None) of the posteriors at the columns of Xs from ONE device call, every sample at its
    own θ."""
    m, _, jx = _device_mean_model(posts).device_means(Xs, [p.slices[0].params for p in posts], api.MEAN_SAMPLE_MAJOR, jac_x=jac_x)
    return m, jx


def _mc_eps(problem: BossProblem, n_posts: int, eps_seed) -> np.ndarray:
    """The ε-samples of expected_improvement(::NonlinFitness): ϵ_sample_count columns for one posterior, one column per posterior
    sample otherwise (expected_improvement.jl:116-119)."""
    count = problem.acquisition.eps_samples if n_posts == 1 else n_posts
    return acq_host.sample_eps(problem.data.Y.shape[0], count, np.random.default_rng(eps_seed))


def acquisition_values(problem: BossProblem, posts: Sequence[HipGaussianProcessPosterior], Xs: np.ndarray,
                       cand: Optional[api.Candidates] = None, eps_seed: Optional[int] = 0, q=None):
    """vals = acq.(eachcol(xs)) for acq = construct_safe_acquisition(problem) — device-evaluated.
    Returns (acq[M], local argmax, local max).  q: a DeviceAcquisition's runtime scalars of this maximisation (default: asked for here)."""
    ei = problem.acquisition
    Xs = np.asfortranarray(Xs, dtype=np.float64)
    if _program_acquisition(problem):
        return _program_values(problem, posts, Xs, cand, ei.scalars(problem) if q is None else q)
    posts, warped = _unwarped(posts)
    if warped:                                               # user-space candidates: the warp runs inside the call
        if cand is not None:
            raise NotImplementedError("resident candidates are not supported for a HipTransformedModel")
        return warped_acquisition_values(problem, posts, Xs)
    own = cand is None
    if own:
        cand = api.Candidates(Xs, problem.model.device)
    constrained = True      # BossProblem.y_max is always a vector (problem.jl:50), Inf entries count as factor 1
    b = best_so_far(ei.fitness, problem.data.Y, problem.y_max)
    mask = None
    if ei.cons_safe:                                                   # make_safe (expected_improvement.jl:58-65)
        mask = in_bounds(Xs, problem.domain.bounds) & in_cons(Xs, problem.domain.cons)
    if isinstance(ei.fitness, DeviceFitness):
        # the closure was traced into a fitness program: the ε-average runs on the device behind the prediction (boss_acq_ei_mc),
        # with the ε draw of the host path below — DeviceFitness(f) and NonlinFitness(f) see identical ε
        eps = _mc_eps(problem, len(posts), eps_seed)
        ym = problem.y_max if constrained else None
        if any(isinstance(s.gp, (api.GibbsGP, api.KernelGP)) for p in posts for s in p.slices):
            # posteriors whose handles boss_acq_ei_mc does not take: their moments, then the Monte-Carlo epilogue on those
            if own:
                cand.close()
            mv = [p.mean_and_var(Xs) for p in posts]
            return api.acq_ei_mc_moments(np.stack([m for m, _ in mv]), np.stack([v for _, v in mv]), ei.fitness.program, eps, ym, b, mask,
                                         problem.model.device)
        gps = [[s.gp for s in p.slices] for p in posts]
        means = None
        if _device_mean_model(posts) is not None:
            means = _device_prior_means(posts, Xs)[0]
        elif posts[0].slices[0]._mean_s(Xs) is not None:
            means = np.stack([np.stack([s._mean_s(Xs) for s in p.slices], axis=0) for p in posts], axis=0)   # S×P×M
        try:
            return api.acq_ei_mc(gps, cand, ei.fitness.program, eps, ym, b, mask, means)
        finally:
            if own:
                cand.close()
    if isinstance(ei.fitness, NonlinFitness):
        # expected_improvement(::NonlinFitness) needs a user closure per Monte-Carlo sample: the device
        # provides (μ, σ²) for every candidate / output / posterior sample, the ε-average runs on the host
        if own:
            cand.close()
        mv = [p.mean_and_var(Xs) for p in posts]
        rng = np.random.default_rng(eps_seed)
        count = ei.eps_samples if len(posts) == 1 else len(posts)      # ϵ_sample_count (expected_improvement.jl:116-117)
        eps = acq_host.sample_eps(problem.data.Y.shape[0], count, rng)
        acq = acq_host.acquisition_nonlin(ei.fitness, mv, problem.y_max if constrained else None, b, eps, mask)
        am = int(np.argmax(acq))
        return acq, am, float(acq[am])
    gps = [[s.gp for s in p.slices] for p in posts]
    means = None
    if _device_mean_model(posts) is not None:
        means = _device_prior_means(posts, Xs)[0]
    elif posts[0].slices[0]._mean_s(Xs) is not None:
        means = np.stack([np.stack([s._mean_s(Xs) for s in p.slices], axis=0) for p in posts], axis=0)   # S×P×M
    acq, am, mx = api.acq_ei(gps, cand, ei.fitness.coefs, problem.y_max if constrained else None, b, mask, means)
    if own:
        cand.close()
    return acq, am, mx


def _program_values(problem: BossProblem, posts, Xs: np.ndarray, cand, q):
    """acquisition_values for a DeviceAcquisition: the traced program behind the prediction in one device call (boss_acq_prog) for
    posteriors of the plain and the gradient-observation model, built-in kernel or DeviceKernel; from the slices' moments
    (boss_acq_prog_moments) for nonstationary posteriors."""
    acq = problem.acquisition
    mask = _program_mask(problem, Xs)
    if any(isinstance(s.gp, api.GibbsGP) for p in posts for s in p.slices):
        mv = [p.mean_and_var(Xs) for p in posts]
        return api.acq_prog_moments(np.stack([m for m, _ in mv]), np.stack([v for _, v in mv]), acq.program, q, mask, acq.outside,
                                    problem.model.device)
    own = cand is None
    if own:
        cand = api.Candidates(Xs, problem.model.device)
    try:
        means = None
        if _device_mean_model(posts) is not None:
            means = _device_prior_means(posts, Xs)[0]
        elif posts[0].slices[0]._mean_s(Xs) is not None:
            means = np.stack([np.stack([s._mean_s(Xs) for s in p.slices], axis=0) for p in posts], axis=0)   # S×P×M
        return api.acq_prog([[s.gp for s in p.slices] for p in posts], cand, acq.program, q, mask, acq.outside, means)
    finally:
        if own:
            cand.close()


@dataclass
class HipBatchAM:
    """x_prior: rng -> x (the reference takes a MultivariateDistribution); points: optional fixed
    d×M grid (GridAM).  samples: number of candidates drawn when `points` is None."""
    x_prior: Optional[Callable] = None
    samples: int = 0
    points: Optional[np.ndarray] = None
    max_attempts: int = 200
    seed: Optional[int] = None
    group: object = None
    shard: str = "candidates"           # "candidates" | "outputs" | "samples"
    fused: bool = True                  # one output, one parameter sample, LinFitness: the posterior update and the acquisition in ONE device
    #                                     call (boss_gp_update_acq: the candidates' substitution rides along the factorisation).  The flag is a
    #                                     permission, on by default: models the fused call does not take — the gradient-observation and
    #                                     nonstationary models, a HipTransformedModel — run the two-call path without an error
    devices: Optional[Sequence[int]] = None   # ONE process driving GPUs 0..G-1: the shard modes run inside the library
    #                                           (boss_multi_*: one host thread per device, exchanges over RCCL) — what a Julia
    #                                           caller uses; None = one process per GPU over torch.distributed (or a single GPU)

    def candidates(self, problem: BossProblem) -> np.ndarray:
        if self.points is not None:
            return np.asfortranarray(self.points, dtype=np.float64)
        rng = np.random.default_rng(dist_util.shared_seed(self.seed, self.group))     # the same draws on every rank
        xs = [_rand_in_domain(self.x_prior, problem.domain, rng, self.max_attempts) for _ in range(self.samples)]
        xs = [x for x in xs if x is not None]                          # _reduce_samples (sampling.jl:77-79)
        if not xs:
            raise RuntimeError("HipBatchAM: No samples were successfully drawn! Check the `x_prior` and the `Domain`.")
        return np.asfortranarray(np.stack(xs, axis=1))

    def maximize_acquisition(self, problem: BossProblem, options: BossOptions = BossOptions(), return_all: bool = False,
                             posts=None):
        """maximize_acquisition(::SamplingAM, problem, options) (sampling.jl:20-40) -> (x, val).
        posts: already-built posteriors of `problem` (HipSequentialBatchAM keeps them resident and
        extends them by block Cholesky appends); default: build them from problem.params."""
        prog = _program_acquisition(problem, "HipBatchAM(devices=[...])" if self.devices is not None else "")
        q = problem.acquisition.scalars(problem) if prog else None      # params(problem): once per maximisation
        Xs = self.candidates(problem)                                   # identical on every rank (seeded)
        M = Xs.shape[1]
        rank, world = dist_util.rank_world(self.group)
        if self.devices is not None or self.shard != "candidates":
            _no_warp(problem, "devices=[...]" if self.devices is not None else f"shard={self.shard!r}")
        if self.devices is not None:
            refuse_device_kernel(problem.model, "HipBatchAM(devices=[...])")
            assert world == 1 and posts is None, "devices=[...] is the single-process mode"
            return self._maximize_in_library(problem, Xs, return_all)
        if self.shard == "outputs":
            return self._maximize_by_outputs(problem, Xs, rank, world, return_all, q)
        if self.shard == "samples":
            return self._maximize_by_samples(problem, Xs, rank, world, return_all, q)
        assert self.shard == "candidates", self.shard
        lo, hi = dist_util.shard_range(M, rank, world)
        if posts is None and self.fused and not prog and hi > lo and self._fusable(problem):
            acq, am, mx = self._update_and_acquire(problem, Xs[:, lo:hi], return_all)
            am += lo
            if return_all:
                return Xs, (dist_util.allgather_concat(acq, self.group) if world > 1 else acq)
            mx, am = dist_util.argmax_exchange(mx, am, self.group)
            return Xs[:, am].copy(), mx
        if posts is None:
            posts = posteriors_of(problem)
        if hi > lo:
            # (q travels only with a DeviceAcquisition: an acquisition_values put in its place by a caller keeps the older signature)
            acq, am, mx = acquisition_values(problem, posts, Xs[:, lo:hi], **({} if q is None else {"q": q}))
            am += lo
        else:
            acq, am, mx = np.zeros(0), M, -np.inf
        if return_all:
            return Xs, (dist_util.allgather_concat(acq, self.group) if world > 1 else acq)
        mx, am = dist_util.argmax_exchange(mx, am, self.group)
        return Xs[:, am].copy(), mx

    @staticmethod
    def _fusable(problem: BossProblem) -> bool:
        """`model_posterior(problem)` is ONE factorisation (one output, one parameter sample) of the plain GP / semiparametric
        model and the acquisition is the analytic EI: the two halves of the BO iteration (src/bo.jl:30-48) fit one device call."""
        from .model import HipGaussianProcess
        return (problem is not None and type(problem.model) is HipGaussianProcess and device_kernel_of(problem.model) is None and
                problem.data.Y.shape[0] == 1 and
                not isinstance(problem.params, (list, tuple)) and not isinstance(problem.acquisition.fitness, NonlinFitness))

    def _update_and_acquire(self, problem: BossProblem, Xs, want_acq: bool):
        """model_posterior(problem) + acq.(eachcol(xs)) + argmax as boss_gp_update_acq: the posterior of the single output is
        built under problem.params while the candidates' forward substitution rides along its factorisation."""
        model, prm, data, ei = problem.model, problem.params, problem.data, problem.acquisition
        Xs = np.asfortranarray(Xs, dtype=np.float64)
        mask = (in_bounds(Xs, problem.domain.bounds) & in_cons(Xs, problem.domain.cons)) if ei.cons_safe else None
        b = best_so_far(ei.fitness, data.Y, problem.y_max)
        g = api.GP(data.X, data.Y[0], model.kernel, model.discrete, model.device)
        cand = api.Candidates(Xs, model.device)
        try:
            if device_mean_of(model) is not None:            # the data's and the candidates' means from one device call
                both = model.mean_values(np.hstack([data.X, Xs]), prm, 0)
                mX, mXs = np.ascontiguousarray(both[:data.X.shape[1]]), np.ascontiguousarray(both[data.X.shape[1]:])
            else:
                mX, mXs = model.mean_values(data.X, prm, 0), model.mean_values(Xs, prm, 0)
            r = g.update_acq(prm.lengthscales[:, 0], prm.amplitudes[0], prm.noise_std[0], cand, fit_coef=float(np.asarray(ei.fitness.coefs)[0]),
                             y_max=float(np.asarray(problem.y_max, float)[0]), best=b, mean_X=mX,
                             mean_Xs=mXs, valid_mask=mask, want_acq=want_acq)
        finally:
            cand.close()
            g.close()
        return r["acq"], r["argmax"], r["max"]

    def _maximize_in_library(self, problem: BossProblem, Xs, return_all):
        """The three shard modes with ONE process driving the devices: posteriors are created on the devices the mode
        assigns them to and the library shards / exchanges itself (boss_multi_acq_ei*)."""
        import dataclasses
        ei = problem.acquisition
        if isinstance(ei.fitness, NonlinFitness):
            raise NotImplementedError("devices=[...] needs the analytic EI of LinFitness")
        devs = list(self.devices)
        G = len(devs)
        if devs != list(range(G)) or api.init() < G:
            raise ValueError("devices must be [0, ..., G-1] with G <= the number of visible GPUs")
        P, S, M = problem.data.Y.shape[0], n_samples(problem), Xs.shape[1]
        plist = list(problem.params) if isinstance(problem.params, (list, tuple)) else [problem.params]
        on = lambda g: dataclasses.replace(problem.model, device=g)
        b = best_so_far(ei.fitness, problem.data.Y, problem.y_max)
        mask = (in_bounds(Xs, problem.domain.bounds) & in_cons(Xs, problem.domain.cons)) if ei.cons_safe else None
        means = None
        if device_mean_of(problem.model) is not None:
            means = problem.model.device_means(Xs, plist)[0]                                                            # S×P×M, one device call
        elif problem.model.mean_values(Xs[:, :1], plist[0], 0) is not None:
            means = np.stack([np.stack([problem.model.mean_values(Xs, prm, i) for i in range(P)]) for prm in plist])   # S×P×M
        slices = []                                                      # everything to close afterwards
        try:
            if self.shard == "candidates":                               # replicas on every device, columns split M/G
                reps = []
                for g in range(G):
                    row = [[on(g).model_posterior_slice(prm, problem.data, i) for i in range(P)] for prm in plist]
                    slices += [sl for r in row for sl in r]
                    reps.append([[sl.gp for sl in r] for r in row])
                acq, am, mx = api.multi_acq_ei(reps, Xs, ei.fitness.coefs, problem.y_max, b, mask, means)
            elif self.shard == "outputs":                                # output i on device i mod G
                row = [[on(dist_util.owner_of(i, G)).model_posterior_slice(prm, problem.data, i) for i in range(P)] for prm in plist]
                slices += [sl for r in row for sl in r]
                acq, am, mx = api.multi_acq_ei_outputs([[sl.gp for sl in r] for r in row], Xs, ei.fitness.coefs, problem.y_max, b, mask, means)
            else:                                                        # sample s on the device of its shard
                assert self.shard == "samples", self.shard
                row = []
                for g in range(G):
                    lo, hi = dist_util.shard_range(S, g, G)
                    row += [[on(g).model_posterior_slice(prm, problem.data, i) for i in range(P)] for prm in plist[lo:hi]]
                slices += [sl for r in row for sl in r]
                acq, am, mx = api.multi_acq_ei_samples([[sl.gp for sl in r] for r in row], Xs, ei.fitness.coefs, problem.y_max, b, mask, means)
        finally:
            for sl in slices:
                sl.close()
        if return_all:
            return Xs, acq
        return Xs[:, am].copy(), mx

    # (the two modes below factorise only a shard of the outputs / samples on each rank)
    def _maximize_by_outputs(self, problem: BossProblem, Xs, rank, world, return_all, q=None):
        if q is None and isinstance(problem.acquisition.fitness, NonlinFitness):   # (q: a DeviceAcquisition, which needs no fitness)
            raise NotImplementedError("shard='outputs' needs the analytic EI of LinFitness; use shard='candidates'")
        P, S, M = problem.data.Y.shape[0], n_samples(problem), Xs.shape[1]
        mine = {i: output_moments(problem, i, Xs) for i in range(P) if dist_util.owner_of(i, world) == rank}
        rows = dist_util.allgather_owned(mine, P, (S, 2, M), self.group)        # [P][S][2][M]
        mu = np.ascontiguousarray(rows[:, :, 0, :].transpose(1, 0, 2))          # [S][P][M]
        var = np.ascontiguousarray(rows[:, :, 1, :].transpose(1, 0, 2))
        acq, am, mx = moments_acquisition(problem, mu, var, Xs, **({} if q is None else {"q": q}))   # identical on every rank
        if return_all:
            return Xs, acq
        return Xs[:, am].copy(), mx

    def _maximize_by_samples(self, problem: BossProblem, Xs, rank, world, return_all, q=None):
        if q is None and isinstance(problem.acquisition.fitness, NonlinFitness):
            raise NotImplementedError("shard='samples' needs the analytic EI of LinFitness; use shard='candidates'")
        S, M = n_samples(problem), Xs.shape[1]
        lo, hi = dist_util.shard_range(S, rank, world)
        part = np.zeros(M)
        if hi > lo:
            posts = posteriors_of(problem, lo, hi)
            acq, _, _ = acquisition_values(problem, posts, Xs, **({} if q is None else {"q": q}))   # mean over the local samples
            part = acq * (hi - lo)
        acq = dist_util.allreduce_sum(part, self.group) / S                      # (:87-90) mean over all samples
        if return_all:
            return Xs, acq
        am = int(np.argmax(acq))                                                 # Julia argmax: first maximum, NaN largest
        return Xs[:, am].copy(), float(acq[am])


@dataclass
class HipSequentialBatchAM:
    """SequentialBatchAM(am, batch_size) (src/acquisition_maximizers/batch.jl:18-38): select
    `batch_size` candidates one after the other, augmenting a COPY of the problem with the
    'speculative' observation (x, posterior mean at x) after each selection.

    The reference rebuilds the posterior from scratch (an O(N^3) Cholesky) for every selected
    point; here the posteriors stay resident and each speculative observation is a block Cholesky
    append (boss_gp_append, O(N^2)) under the unchanged hyper-parameters — same posterior.  When the
    inner maximiser's candidate set is fixed (`points`, or a seeded sample) the candidates' predictive
    state stays resident too (boss_track_*) and is extended in O(N·M) per selection.  A model under a DeviceKernel takes both
    routes when the kernel was traced with sequential=True (boss_kgp_set_sequential), and raises NotImplementedError otherwise."""
    am: HipBatchAM
    batch_size: int

    def maximize_acquisition(self, problem: BossProblem, options: BossOptions = BossOptions()):
        import copy
        if int(self.batch_size) < 1:
            raise ValueError(f"HipSequentialBatchAM: batch_size = {self.batch_size}, at least one point is selected")
        _no_warp(problem, "HipSequentialBatchAM (appending observations, tracked candidates)")
        refuse_device_kernel(problem.model, "HipSequentialBatchAM (appending observations, tracked candidates)", seq_ok=True)
        prob = copy.copy(problem)                                        # problem_ = deepcopy(problem) (batch.jl:27)
        prob.data = type(problem.data)(problem.data.X.copy(), problem.data.Y.copy())
        posts = posteriors_of(prob, reserve=self.batch_size)             # no re-allocation when the appends arrive
        fixed = self.am.points is not None or self.am.seed is not None   # same candidate set at every selection
        # (a DeviceAcquisition takes the untracked loop a NonlinFitness takes: the tracks know the EI epilogue alone)
        lin = not _program_acquisition(prob) and not isinstance(prob.acquisition.fitness, NonlinFitness)
        try:
            if fixed and lin and self.am.shard == "candidates":
                return self._tracked(prob, posts), None
            xs = []
            for _ in range(self.batch_size):                             # speculative_evaluation! (batch.jl:32-38)
                x, _ = self.am.maximize_acquisition(prob, options, posts=posts)
                y = sum(p.mean(x) for p in posts) / len(posts)           # mean(post, x); BI: average_mean
                prob.augment_dataset(x, y)
                for p in posts:
                    p.append(x, y)
                xs.append(x)
            return np.stack(xs, axis=1), None
        finally:
            for p in posts:
                p.close()

    def _tracked(self, prob: BossProblem, posts):
        """Fixed candidate set: the candidates' V slabs stay resident (api.Track) and every speculative
        observation extends them by one row — O(N·M) per selection instead of the O(N²M) re-solve."""
        Xs = self.am.candidates(prob)                                    # identical on every rank
        M = Xs.shape[1]
        rank, world = dist_util.rank_world(self.am.group)
        lo, hi = dist_util.shard_range(M, rank, world)
        ei = prob.acquisition
        dev = prob.model.device
        cand = api.Candidates(Xs[:, lo:hi], dev) if hi > lo else None
        tracks = []
        if cand is not None and _device_mean_model(posts) is not None:
            mm = _device_prior_means(posts, Xs[:, lo:hi])[0]
            tracks = [[api.Track(s.gp, cand, np.ascontiguousarray(mm[k, i])) for i, s in enumerate(p.slices)] for k, p in enumerate(posts)]
        elif cand is not None:
            tracks = [[api.Track(s.gp, cand, s._mean_s(Xs[:, lo:hi])) for s in p.slices] for p in posts]
        mask = None
        if ei.cons_safe and hi > lo:
            mask = in_bounds(Xs[:, lo:hi], prob.domain.bounds) & in_cons(Xs[:, lo:hi], prob.domain.cons)
        xs = []
        try:
            for _ in range(self.batch_size):
                b = best_so_far(ei.fitness, prob.data.Y, prob.y_max)
                if cand is not None:
                    _, am, mx = api.acq_ei_tracks(tracks, ei.fitness.coefs, prob.y_max, b, mask, want_acq=False)
                    am += lo
                else:
                    am, mx = M, -np.inf
                mx, am = dist_util.argmax_exchange(mx, am, self.am.group)
                x = Xs[:, am].copy()
                yl = None
                if lo <= am < hi:                                        # the owner reads ŷ = mean(post, x) off its tracks
                    yl = sum(np.array([t.moments(am - lo, 1)[0][0] for t in ts]) for ts in tracks) / len(tracks)
                P = prob.data.Y.shape[0]                                 # one fixed-size broadcast from the owner
                y = dist_util.broadcast_array(yl, (P,), dist_util.owner_of_index(am, M, world), self.am.group) if world > 1 else yl
                prob.augment_dataset(x, y)
                for p in posts:
                    p.append(x, y)
                xs.append(x)
        finally:
            for ts in tracks:
                for t in ts:
                    t.close()
            if cand is not None:
                cand.close()
        return np.stack(xs, axis=1)


@dataclass
class HipGradientAM:
    """OptimizationAM semantics (src/acquisition_maximizers/optimization.jl:13-118): multistart LOCAL
    optimisation of the acquisition, started from `multistart` x_prior samples inside the domain, the
    best local optimum wins (optim_multistart.jl).  The reference differentiates the acquisition with
    ForwardDiff (optimization.jl:36) one start at a time; here the gradient is analytic and evaluated
    on the device (boss_acq_ei_grad; boss_acq_ei_grad_set for the S samples of a BI fit) for ALL starts in one call per
    iteration: projected gradient
    ascent with a per-start Barzilai–Borwein step and backtracking.  Discrete dimensions are rounded
    (their gradient is zero), `cons` is honoured through make_safe (acq = 0 outside) and a final
    in-domain filter.  Multi-GPU: the starts are sharded across ranks, 16-byte arg-max exchange.
    `mean_grad`: optional x -> P×d Jacobian of the GP's prior mean (zero / constant means need none).  A model whose mean is a
    DeviceMean needs none either: ∂m/∂x comes from the traced program at every iteration, every parameter sample at its own θ, in the
    device call that gives the mean values; giving `mean_grad` as well raises ValueError."""
    x_prior: Callable = None
    multistart: int = 200
    iters: int = 30
    max_attempts: int = 200
    seed: Optional[int] = None
    group: object = None
    mean_grad: Optional[Callable] = None
    eps_seed: Optional[int] = 0         # DeviceFitness: the ε-samples are drawn once per maximize_acquisition call (common random
    #                                     numbers across the iterations: the ascent climbs ONE deterministic surface)

    def _eps(self, problem: BossProblem, n_posts: int) -> np.ndarray:
        """The ε-samples of this maximize_acquisition call (drawn at its first use, kept until the next call begins)."""
        key = (problem.data.Y.shape[0], problem.acquisition.eps_samples if n_posts == 1 else n_posts)
        cache = self.__dict__.setdefault("_eps_cache", {})
        if key not in cache:
            cache[key] = _mc_eps(problem, n_posts, self.eps_seed)
        return cache[key]

    def _value_and_grad(self, problem: BossProblem, posts, X):
        posts, warped = _unwarped(posts)
        if warped:
            if self.mean_grad is not None:
                raise ValueError("HipGradientAM: mean_grad is not taken for a HipTransformedModel (a DeviceMean gives its own ∂m/∂x_)")
            return warped_value_and_grad(problem, posts, X)
        ei = problem.acquisition
        if _program_acquisition(problem):
            return self._program_value_and_grad(problem, posts, X)
        mc = isinstance(ei.fitness, DeviceFitness)
        if isinstance(ei.fitness, NonlinFitness) and not mc:
            raise NotImplementedError("HipGradientAM needs the analytic EI of LinFitness, or a DeviceFitness")
        b = best_so_far(ei.fitness, problem.data.Y, problem.y_max)
        mask = (in_bounds(X, problem.domain.bounds) & in_cons(X, problem.domain.cons)) if ei.cons_safe else None
        M = X.shape[1]
        eps = self._eps(problem, len(posts)) if mc else None
        mg = None                                            # P×d×M Jacobian of the prior mean: the same for every sample
        dev = _device_mean_model(posts) is not None
        if dev and self.mean_grad is not None:
            raise ValueError("HipGradientAM: the model's mean is a DeviceMean, which gives its own ∂m/∂x; drop mean_grad")
        if self.mean_grad is not None:
            mg = np.stack([np.asarray(self.mean_grad(X[:, j]), float) for j in range(M)], axis=2)
        if dev:
            # DeviceMean: S×P×M means and S×P×d×M ∂m/∂x of all samples and outputs at their own θ from one device call
            dms, dmg = _device_prior_means(posts, X, jac_x=True)
            gps = [[s.gp for s in post.slices] for post in posts]
            if mc:
                return api.acq_ei_mc_grad(gps, X, ei.fitness.program, eps, problem.y_max, b, mask, dms, dmg)
            if len(posts) > 1:
                return api.acq_ei_grad_set(gps, X, ei.fitness.coefs, problem.y_max, b, mask, dms, dmg)
            return api.acq_ei_grad(gps[0], X, ei.fitness.coefs, problem.y_max, b, mask, dms[0], dmg[0])

        def means(post):                                     # P×M prior means of one sample, or None when no slice has one
            rows = [s._mean_s(X) for s in post.slices]
            if all(r is None for r in rows):
                return None
            return np.stack([np.zeros(M) if r is None else np.asarray(r, float) for r in rows])

        nonstat = any(isinstance(s.gp, api.GibbsGP) for post in posts for s in post.slices)
        if mc and nonstat:
            # nonstationary posteriors: every slice's moments and moment gradients, then the Monte-Carlo chain rule on those
            # (boss_acq_ei_mc_grad_moments sums the samples in ascending order)
            mvg = [[s.mean_and_var_grad(X) if mg is None else s.mean_and_var_grad(X, mean_grad=mg[i]) for i, s in enumerate(post.slices)]
                   for post in posts]
            mu, var, dmu, dvar = (np.stack([np.stack([r[q] for r in row]) for row in mvg]) for q in range(4))
            return api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, ei.fitness.program, eps, problem.y_max, b, mask, problem.model.device)
        if mc:
            # the Monte-Carlo EI of the traced program and its gradient in ONE device call, one sample or many (boss_acq_ei_mc_grad)
            mm = [means(post) for post in posts]
            ms = None
            if any(m is not None for m in mm):
                ms = np.stack([np.zeros((len(post.slices), M)) if m is None else m for m, post in zip(mm, posts)])
            mgs = None if mg is None else np.stack([mg] * len(posts))
            return api.acq_ei_mc_grad([[s.gp for s in post.slices] for post in posts], X, ei.fitness.program, eps, problem.y_max, b, mask,
                                      ms, mgs)
        if len(posts) > 1 and not nonstat:
            # BI: the sample mean of the acquisition and of its gradient in ONE device call (boss_acq_ei_grad_set)
            mm = [means(post) for post in posts]
            ms = None
            if any(m is not None for m in mm):               # samples without a prior mean travel as zeros
                ms = np.stack([np.zeros((len(post.slices), M)) if m is None else m for m, post in zip(mm, posts)])   # S×P×M
            mgs = None if mg is None else np.stack([mg] * len(posts))                                              # S×P×d×M
            return api.acq_ei_grad_set([[s.gp for s in post.slices] for post in posts], X, ei.fitness.coefs, problem.y_max, b,
                                       mask, ms, mgs)
        acc, gacc = 0.0, 0.0
        for post in posts:                                   # one sample (MAP), or nonstationary models: sample by sample
            a, g = api.acq_ei_grad([s.gp for s in post.slices], X, ei.fitness.coefs, problem.y_max, b, mask, means(post), mg)
            acc, gacc = acc + a, gacc + g
        return acc / len(posts), gacc / len(posts)

    def _program_value_and_grad(self, problem: BossProblem, posts, X):
        """A DeviceAcquisition: the traced program and its reverse sweep behind the moment gradients in ONE device call, one sample
        or many (boss_acq_prog_grad); from the slices' moments and moment gradients for nonstationary posteriors."""
        acq = problem.acquisition
        q = self.__dict__.get("_acq_q")
        if q is None:                                        # (called outside maximize_acquisition)
            q = acq.scalars(problem)
        mask = _program_mask(problem, X)
        M = X.shape[1]
        gps = [[s.gp for s in post.slices] for post in posts]
        dev = _device_mean_model(posts) is not None
        if dev and self.mean_grad is not None:
            raise ValueError("HipGradientAM: the model's mean is a DeviceMean, which gives its own ∂m/∂x; drop mean_grad")
        if dev:
            dms, dmg = _device_prior_means(posts, X, jac_x=True)
            return api.acq_prog_grad(gps, X, acq.program, q, mask, acq.outside, dms, dmg)
        mg = None
        if self.mean_grad is not None:
            mg = np.stack([np.asarray(self.mean_grad(X[:, j]), float) for j in range(M)], axis=2)
        if any(isinstance(s.gp, api.GibbsGP) for post in posts for s in post.slices):
            mvg = [[s.mean_and_var_grad(X) if mg is None else s.mean_and_var_grad(X, mean_grad=mg[i]) for i, s in enumerate(post.slices)]
                   for post in posts]
            mu, var, dmu, dvar = (np.stack([np.stack([r[k] for r in row]) for row in mvg]) for k in range(4))
            return api.acq_prog_grad_moments(mu, var, dmu, dvar, acq.program, q, mask, acq.outside, problem.model.device)
        rows = [[s._mean_s(X) for s in post.slices] for post in posts]
        ms = None
        if any(r is not None for row in rows for r in row):  # slices without a prior mean travel as zeros
            ms = np.stack([np.stack([np.zeros(M) if r is None else np.asarray(r, float) for r in row]) for row in rows])   # S×P×M
        mgs = None if mg is None else np.stack([mg] * len(posts))
        return api.acq_prog_grad(gps, X, acq.program, q, mask, acq.outside, ms, mgs)

    def maximize_acquisition(self, problem: BossProblem, options: BossOptions = BossOptions(), posts=None):
        refuse_device_kernel(problem.model, "HipGradientAM (candidate gradients)", grad_ok=True)
        self.__dict__.pop("_acq_q", None)
        if _program_acquisition(problem):
            self.__dict__["_acq_q"] = problem.acquisition.scalars(problem)   # params(problem): once per maximisation
        try:
            return self._maximize(problem, posts)
        finally:
            self.__dict__.pop("_acq_q", None)                # (a later _value_and_grad call asks params(problem) itself)

    def _maximize(self, problem: BossProblem, posts):
        if isinstance(getattr(problem.acquisition, "fitness", None), DeviceFitness):
            refuse_device_kernel(problem.model, "HipGradientAM with a DeviceFitness (Monte-Carlo EI gradients are built-in-kernel only)")
        if self.mean_grad is not None and device_mean_of(problem.model) is not None:
            raise ValueError("HipGradientAM: the model's mean is a DeviceMean, which gives its own ∂m/∂x; drop mean_grad")
        rng = np.random.default_rng(dist_util.shared_seed(self.seed, self.group))     # the same starts on every rank
        dom = problem.domain
        starts = [_rand_in_domain(self.x_prior, dom, rng, self.max_attempts) for _ in range(self.multistart)]
        starts = [x for x in starts if x is not None]
        if not starts:
            raise RuntimeError("HipGradientAM: No samples were successfully drawn! Check the `x_prior` and the `Domain`.")
        X0 = np.asfortranarray(np.stack(starts, axis=1))
        rank, world = dist_util.rank_world(self.group)
        lo, hi = dist_util.shard_range(X0.shape[1], rank, world)
        if posts is None:
            posts = posteriors_of(problem)
        best_v, best_i, Xf = -np.inf, X0.shape[1], None
        if hi > lo:
            X = X0[:, lo:hi].copy()
            lb, ub = dom.bounds
            span = np.where(np.isfinite(ub - lb), ub - lb, 1.0)[:, None]
            cont = ~dom.discrete
            self.__dict__.pop("_eps_cache", None)           # a DeviceFitness draws its ε-samples once per call, at the first evaluation
            f, g = self._value_and_grad(problem, posts, X)
            step = np.full(X.shape[1], 0.05)                 # relative to the box, per start
            for _ in range(self.iters):
                gn = g * span
                gn[~cont] = 0.0
                nrm = np.maximum(np.sqrt((gn * gn).sum(0)), 1e-300)
                Xn = X + (gn / nrm) * span * step[None, :]
                Xn = np.minimum(np.maximum(Xn, lb[:, None]), ub[:, None])
                fn, gnw = self._value_and_grad(problem, posts, Xn)
                better = fn > f
                X[:, better], f[better], g[:, better] = Xn[:, better], fn[better], gnw[:, better]
                step = np.where(better, np.minimum(step * 1.5, 0.5), step * 0.4)
                if np.all(step < 1e-7):
                    break
            ok = in_domain(X, dom)
            fm = np.where(ok, f, -np.inf)
            j = int(np.argmax(fm))
            best_v, best_i, Xf = float(fm[j]), lo + j, X
        best_v, gi = dist_util.argmax_exchange(best_v, best_i, self.group)
        if world > 1:                                        # the winner's refined point: one d-double broadcast from its owner
            owner = dist_util.owner_of_index(gi, X0.shape[1], world)
            mine = Xf[:, gi - lo] if owner == rank else None
            return dist_util.broadcast_array(mine, (X0.shape[0],), owner, self.group), best_v
        return Xf[:, gi - lo].copy(), best_v
