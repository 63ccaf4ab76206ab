"""Gradients of program-kernel posteriors on the device (boss_kgp_set_grad, B.DeviceKernel(..., grad=True)): likelihood gradient,
moment gradients on every adjoint-substitution route, acquisition gradients, and the three gradient-based plugins.

Expected values: kernel_grad_cases.RestatedGrad — closed-form partials of the closures, K⁻¹ and K⁻¹K* by scipy solves.
Tolerance: the project's bar for built-in gradients on comparable inputs (test_loglike_gradient / test_predict_grad of
tests/test_gpu_parity.py), atol = 1e-8·(1 + max|want|), widened to max(1e-8, ref.tol)·(1 + max|want|) with the restatement's
tol = max(1e-9, cond(K)·N·2⁻⁵³·8).  Every input keeps cond(K) below 1e6 (asserted).  On the built-in closures (matern32, matern52,
sqexp) the built-in handle's error against the same truth is printed beside the program handle's; where the built-in handle itself
misses the bar, the bar of that quantity is 4× the built-in handle's measured error (`bar`).

Shapes, each the smallest that can fail in its way:
  n20     N = 20,   d = 1,  M = 5      below SMALL_MAX_N: must not take the one-launch small paths of the built-in kernels
  n130    N = 130,  d = 3,  M = 70     diagonal, off-diagonal and ragged 64×64 tiles; a ragged candidate tile; split rows (3 tiles)
  n130dm  the same with a discrete dimension, a prior mean and its gradient: the discrete rows of ∇μ, ∇σ² are exactly 0
  n130w   N = 130,  d = 16, M = 33     persq: values plus adjoints of its program exceed 64 KiB per wave
  n130b   N = 130,  d = 3,  M = 4101   129 candidate tiles: the unsplit accumulation
  n1030   N = 1030, d = 3,  M = 40     the step-by-step adjoint route, then the resident-inverse GEMM (winv_after + 2 calls)"""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_program_cases as cases  # noqa: E402
import kernel_grad_cases as gcases  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {
    "n20": dict(d=1, N=20, M=5),
    "n130": dict(d=3, N=130, M=70),
    "n130dm": dict(d=3, N=130, M=70, discrete=[False, True, False], scale=[1.0, 4.0, 1.0], mean=True),
    "n130w": dict(d=16, N=130, M=33),
    "n130b": dict(d=3, N=130, M=4101),
    "n1030": dict(d=3, N=1030, M=40),
}
AMP = 1.0
NAMES = sorted(gcases.ALL)
CASES = ([(s, n) for s in ("n20", "n130", "n130dm") for n in NAMES] + [("n130w", "persq")] +
         [("n130b", n) for n in ("dot1", "expo", "matern52")])


def noise_of(name):
    """σ >= 0.05; the dot-product kernel's largest eigenvalue grows like N(1 + |u|²), so it takes σ = 0.1 to stay below cond 1e6."""
    return 0.1 if name == "dot1" else 0.05


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    B.api.load_library()
    assert B.api.device_count() >= 1
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


_kernels, _refs = {}, {}


def kernel_of(B, name, d, grad=True):
    if (name, d, grad) not in _kernels:
        _kernels[(name, d, grad)] = B.DeviceKernel(gcases.ALL[name], d, grad=grad)
    return _kernels[(name, d, grad)]


def setup(shape, name):
    """(X, y, Xs, lam, sig, discrete, mean_X, mean_Xs, mean_grad, restatement, second member's restatement), computed once."""
    key = (shape, name)
    if key not in _refs:
        s = SHAPES[shape]
        d, sc = s["d"], np.asarray(s.get("scale", np.ones(s["d"])), float)
        X, y, Xs = cases.data(d, s["N"], s["M"], seed=3, scale=sc)
        lam = np.linspace(0.4, 0.6, d) * sc
        disc = s.get("discrete")
        mX = mXs = mg = None
        if s.get("mean"):                                    # m(x) = 0.5 + 0.2 Σ_{k not discrete} x_k: no gradient along a discrete dimension
            live = ~np.asarray(disc, bool)
            mX, mXs = 0.5 + 0.2 * X[live].sum(0), 0.5 + 0.2 * Xs[live].sum(0)
            mg = np.repeat(np.where(live, 0.2, 0.0)[:, None], s["M"], axis=1)
        f = gcases.ALL[name]
        ref = gcases.RestatedGrad(f, X, y, lam, AMP, noise_of(name), Xs, disc, mX, mXs, mg)
        ref2 = gcases.RestatedGrad(f, X, y, lam * 1.15, AMP, noise_of(name) * 1.2, Xs, disc, mX, mXs, mg, want_cond=False)
        for a in (X, y, Xs, ref.mu, ref.var, ref.dmu, ref.dvar, ref.dlogpdf, ref.a):
            a.setflags(write=False)
        _refs[key] = (X, y, Xs, lam, noise_of(name), disc, mX, mXs, mg, ref, ref2)
    return _refs[key]


def bar(want, ref, builtin_err=None):
    b = max(1e-8, ref.tol) * (1 + np.abs(want).max())
    if builtin_err is not None and builtin_err > b:          # the built-in handle misses the bar itself: 4× its measured error
        b = 4.0 * builtin_err
    return b


def held(tag, what, got, want, ref, got_builtin=None):
    err = np.abs(np.asarray(got) - want).max()
    eb = None if got_builtin is None else np.abs(np.asarray(got_builtin) - want).max()
    b = bar(want, ref, eb)
    print(f"[kgrad] {tag} {what}: err {err:.3e} (bound {b:.3e})" + ("" if eb is None else f" built-in handle {eb:.3e}"))
    assert err <= b, (tag, what, err, b)


def ei_want(O, refs, best):
    """mean over the members of EI and ∇EI from the restatements' moments (LinFitness [1.0], no constraint)."""
    acc, gacc = 0.0, 0.0
    for r in refs:
        var = np.where((r.var < 0.0) & (r.var >= -1e-8), 0.0, r.var)
        a, g = O.expected_improvement_lin_grad([1.0], r.mu[None], var[None], r.dmu[None], np.where(var > 0, r.dvar, 0.0)[None], best)
        acc, gacc = acc + a, gacc + g
    return acc / len(refs), gacc / len(refs)


def mean_args(mXs, mg, members):
    return (None if mXs is None else np.stack([mXs[None]] * members), None if mg is None else np.stack([mg[None]] * members))


@pytest.mark.parametrize("shape,name", CASES)
def test_gradients_match_the_restatement(B, api, O, shape, name):
    X, y, Xs, lam, sig, disc, mX, mXs, mg, ref, ref2 = setup(shape, name)
    d = X.shape[0]
    tag = f"{shape} {name}"
    assert ref.cond < 1e6
    prog = kernel_of(B, name, d).program
    g = api.KernelGP(X, y, prog, disc, grad=True)
    g2 = api.KernelGP(X, y, prog, disc)
    assert api.load_library().boss_kgp_set_grad(g2._h, 1) == api.BOSS_OK       # the switch after creation, before the update
    gu = api.KernelGP(X, y, prog, disc)                      # unflagged, on the same context
    gb = api.GP(X, y, name, disc) if name in cases.BUILTIN else None
    try:
        lp = g.update(lam, AMP, sig, mX)
        g2.update(lam * 1.15, AMP, sig * 1.2, mX)
        gu.update(lam, AMP, sig, mX)
        if gb is not None:
            gb.update(lam, AMP, sig, mX)
        # likelihood gradient, and dmean = a
        lp1, grad = g.loglike_grad()
        lp2, grad2, dmean = g.loglike_grad_mean()
        assert lp1 == lp and lp2 == lp and np.array_equal(grad, grad2)
        assert abs(lp - ref.logpdf) <= ref.tol * (1 + abs(ref.logpdf))
        held(tag, "dlogpdf", grad, ref.dlogpdf, ref, None if gb is None else gb.loglike_grad()[1])
        held(tag, "dmean", dmean, ref.a, ref, None if gb is None else gb.loglike_grad_mean()[2])
        assert np.array_equal(g.loglike_grad()[1], grad)     # no atomics: repeated calls agree bit for bit
        # moment gradients
        mu, var, dmu, dvar = g.predict_grad(Xs, mXs, mg)
        pb = None if gb is None else gb.predict_grad(Xs, mXs, mg)
        held(tag, "mu", mu, ref.mu, ref, None if pb is None else pb[0])
        held(tag, "var", var, ref.var, ref, None if pb is None else pb[1])
        held(tag, "dmu", dmu, ref.dmu, ref, None if pb is None else pb[2])
        held(tag, "dvar", dvar, ref.dvar, ref, None if pb is None else pb[3])
        if disc is not None:
            k = int(np.flatnonzero(disc)[0])
            assert not dmu[k].any() and not dvar[k].any()
        again = g.predict_grad(Xs, mXs, mg)
        assert all(np.array_equal(a, b) for a, b in zip((mu, var, dmu, dvar), again))
        # acquisition gradient, one member and two
        best = float(np.median(ref.mu))
        m1, g1 = mean_args(mXs, mg, 1)
        acq, dacq = api.acq_ei_grad([g], Xs, [1.0], None, best, None, None if m1 is None else m1[0], None if g1 is None else g1[0])
        want, dwant = ei_want(O, [ref], best)
        ab = None
        if gb is not None:
            ab = api.acq_ei_grad([gb], Xs, [1.0], None, best, None, None if m1 is None else m1[0], None if g1 is None else g1[0])
        held(tag, "acq", acq, want, ref, None if ab is None else ab[0])
        held(tag, "dacq", dacq, dwant, ref, None if ab is None else ab[1])
        m2, gm2 = mean_args(mXs, mg, 2)
        acq_s, dacq_s = api.acq_ei_grad_set([[g], [g2]], Xs, [1.0], None, best, None, m2, gm2)
        want_s, dwant_s = ei_want(O, [ref, ref2], best)
        held(tag, "acq set", acq_s, want_s, ref)
        held(tag, "dacq set", dacq_s, dwant_s, ref)
        acq_r, dacq_r = api.acq_ei_grad_set([[g], [g2]], Xs, [1.0], None, best, None, m2, gm2)
        assert np.array_equal(acq_r, acq_s) and np.array_equal(dacq_r, dacq_s)
        # an unflagged handle next to it is refused as before, alone or mixed with a flagged one
        for call in (gu.loglike_grad, gu.loglike_grad_mean, lambda: gu.predict_grad(Xs[:, :3]),
                     lambda: api.acq_ei_grad([gu], Xs[:, :3], [1.0], None, best),
                     lambda: api.acq_ei_grad([g, gu], Xs[:, :3], [1.0, 0.0], None, best),
                     lambda: api.acq_ei_grad_set([[g], [gu]], Xs[:, :3], [1.0], None, best)):
            with pytest.raises(api.BossError) as e:
                call()
            assert e.value.code == api.BOSS_E_INVALID and "program-kernel posteriors" in str(e.value)
        # the switch goes off again; nothing resident changed
        assert api.load_library().boss_kgp_set_grad(g2._h, 0) == api.BOSS_OK
        with pytest.raises(api.BossError):
            g2.loglike_grad()
        assert np.array_equal(g.predict_grad(Xs, mXs, mg)[2], dmu)
    finally:
        for h in (g, g2, gu, gb):
            if h is not None:
                h.close()


@pytest.mark.parametrize("name", ["expo", "matern52"])
def test_adjoint_routes_of_the_few_candidates_path(B, api, O, name):
    """N = 1030 (Np = 1280), M = 40: calls 1 .. winv_after - 1 on one factorisation take the step-by-step adjoint substitution
    (few_back_*), from call winv_after on both inverse factors are resident and W = L⁻ᵀV is one GEMM (inv_bwd_kernel).  The route is
    read from the handle as tests/test_gpu_kernel_program.py reads it."""
    for knob in ("BOSS_INVGEMM_MAX_TILES", "BOSS_FEW_MAX_TILES", "BOSS_NO_FEW"):
        assert os.environ.get(knob) is None, knob + " is set: this test would not reach the resident-inverse route"
    winv_after = int(os.environ.get("BOSS_WINV_AFTER", "2"))
    assert winv_after >= 1
    X, y, Xs, lam, sig, disc, mX, mXs, mg, ref, ref2 = setup("n1030", name)
    assert ref.cond < 1e6
    g = api.KernelGP(X, y, kernel_of(B, name, 3).program, grad=True)
    gb = api.GP(X, y, name) if name in cases.BUILTIN else None
    try:
        lp = g.update(lam, AMP, sig)
        if gb is not None:
            gb.update(lam, AMP, sig)
        assert api._acq_counters(g)[:2] == (0, 0)
        _, grad = g.loglike_grad()
        held(f"n1030 {name}", "dlogpdf", grad, ref.dlogpdf, ref, None if gb is None else gb.loglike_grad()[1])
        best = float(np.median(ref.mu))
        want, dwant = ei_want(O, [ref], best)
        for rep in range(winv_after + 2):
            mu, var, dmu, dvar = g.predict_grad(Xs)
            have_winv, few_calls = api._acq_counters(g)[:2]
            assert have_winv == (1 if rep + 1 >= winv_after else 0) and few_calls == min(rep + 1, winv_after), (rep, have_winv, few_calls)
            pb = None if gb is None else gb.predict_grad(Xs)
            tag = f"n1030 {name} call {rep} ({'inverse GEMM' if have_winv else 'steps'})"
            held(tag, "dmu", dmu, ref.dmu, ref, None if pb is None else pb[2])
            held(tag, "dvar", dvar, ref.dvar, ref, None if pb is None else pb[3])
        acq, dacq = api.acq_ei_grad([g], Xs, [1.0], None, best)
        ab = None if gb is None else api.acq_ei_grad([gb], Xs, [1.0], None, best)
        held(f"n1030 {name}", "acq", acq, want, ref, None if ab is None else ab[0])
        held(f"n1030 {name}", "dacq", dacq, dwant, ref, None if ab is None else ab[1])
    finally:
        g.close()
        if gb is not None:
            gb.close()


@pytest.mark.parametrize("shape", ["n130", "n130dm"])
def test_a_candidate_on_a_training_point(B, api, shape):
    """matern52 spelled as a program, one candidate placed on a training point (r = 0 in the reverse sweep: SQRT'(0) = +Inf meets
    SQUARE' = 0): finite gradients that agree with the built-in matern52 handle within the bar."""
    X, y, Xs, lam, sig, disc, mX, mXs, mg, ref, _ = setup(shape, "matern52")
    Xc = np.array(Xs[:, :40])
    Xc[:, 5] = X[:, 17]
    mc = None if mXs is None else 0.5 + 0.2 * Xc[~np.asarray(disc, bool)].sum(0)
    gc = None if mg is None else mg[:, :40]
    g = api.KernelGP(X, y, kernel_of(B, "matern52", 3).program, disc, grad=True)
    gb = api.GP(X, y, "matern52", disc)
    try:
        g.update(lam, AMP, sig, mX)
        gb.update(lam, AMP, sig, mX)
        got, want = g.predict_grad(Xc, mc, gc), gb.predict_grad(Xc, mc, gc)
        assert all(np.all(np.isfinite(a)) for a in got)
        for what, a, b in zip(("mu", "var", "dmu", "dvar"), got, want):
            held(f"{shape} on a training point", what, a, b, ref)
        best = float(np.median(ref.mu))
        m_ = None if mc is None else mc[None]
        g_ = None if gc is None else gc[None]
        (a1, d1), (a2, d2) = api.acq_ei_grad([g], Xc, [1.0], None, best, None, m_, g_), api.acq_ei_grad([gb], Xc, [1.0], None, best, None, m_, g_)
        assert np.all(np.isfinite(d1))
        held(f"{shape} on a training point", "acq", a1, a2, ref)
        held(f"{shape} on a training point", "dacq", d1, d2, ref)
    finally:
        g.close()
        gb.close()


@pytest.mark.parametrize("name", ["dot1", "expo", "persq"])
def test_directional_difference_of_the_devices_own_likelihood(B, api, name):
    """As test_full_size_next_rows of tests/test_gpu_parity.py: central differences (ε = 1e-5) of update()'s logpdf along λ_1, λ_d, α and
    σ against loglike_grad, within that test's 2e-5·(1 + |want|)."""
    X, y, Xs, lam, sig, disc, mX, *_ = setup("n130dm", name)
    d = 3
    g = api.KernelGP(X, y, kernel_of(B, name, d).program, disc, grad=True)
    try:
        g.update(lam, AMP, sig, mX)
        _, grad = g.loglike_grad()
        eps = 1e-5
        for k, (dl, da, ds) in enumerate([(np.eye(d)[0], 0, 0), (np.eye(d)[d - 1], 0, 0), (np.zeros(d), 1, 0), (np.zeros(d), 0, 1)]):
            fp = g.update(lam + eps * dl, AMP + eps * da, sig + eps * ds, mX)
            fm = g.update(lam - eps * dl, AMP - eps * da, sig - eps * ds, mX)
            want, got = (fp - fm) / (2 * eps), grad[[0, d - 1, d, d + 1][k]]
            print(f"[kgrad] own likelihood {name} direction {k}: gradient {got:.6e} differences {want:.6e}")
            assert abs(got - want) <= 2e-5 * (1 + abs(want)), (k, got, want)
    finally:
        g.close()


def _problem(B, dk, theta=False):
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (2, 24))
    Y = (np.sin(3.0 * X[0]) + np.cos(2.0 * X[1]))[None, :]
    pri = dict(lengthscale_priors=[B.MvLogNormal(np.log([0.5, 0.5]), [0.2, 0.2])], amplitude_priors=[B.LogNormal(0.0, 0.2)],
               noise_std_priors=[B.Dirac(0.05)])
    model = B.HipGaussianProcess(kernel=dk, **pri)
    f = lambda x: [np.sin(3.0 * x[0]) + np.cos(2.0 * x[1])]
    return B.BossProblem(f, B.Domain(([0.0, 0.0], [1.0, 1.0])), B.ExpectedImprovement(B.LinFitness([1.0])), model, B.ExperimentData(X, Y))


def _log_posterior(prob, p):
    ll = prob.model.data_loglike(prob.data)
    try:
        return ll(p) + prob.model.params_loglike()(p)
    finally:
        for h in ll.handles:
            h.close()


def test_gradient_map_never_ends_below_its_start(B):
    """HipGradientMAP on the 24-point problem of the surface test of tests/test_gpu_kernel_program.py, exponential kernel with
    gradients: every start ends at a log-posterior no lower than it began with, and the model's gradient calls agree with each other."""
    prob = _problem(B, kernel_of(B, "expo", 2))
    sampler = prob.model.params_sampler()
    rng = np.random.default_rng(5)
    starts = [sampler(rng) for _ in range(4)]
    before = [_log_posterior(prob, p) for p in starts]
    res = B.HipGradientMAP(4, 6, seed=0, starts=starts).estimate_parameters(prob, return_all=True)
    assert len(res) == 4
    for k, r in enumerate(res):
        print(f"[kgrad] HipGradientMAP start {k}: {before[k]:.6f} -> {r.loglike:.6f}")
        assert r.loglike >= before[k]
        assert abs(_log_posterior(prob, r.params) - r.loglike) <= 1e-9 * (1 + abs(r.loglike))
    assert any(r.loglike > b for r, b in zip(res, before))
    best = B.HipGradientMAP(4, 6, seed=0, starts=starts).estimate_parameters(prob)
    assert best.loglike == max(r.loglike for r in res)
    # data_loglike_grad_batch: an invalid set is a sample of likelihood -inf with zero gradients
    bad = B.HipGPParams(starts[0].lengthscales, -starts[0].amplitudes, starts[0].noise_std)
    lls, grads = prob.model.data_loglike_grad_batch(prob.data, [starts[0], bad, starts[1]])
    assert np.isfinite(lls[0]) and lls[1] == -np.inf and np.isfinite(lls[2])
    assert not grads[1].lengthscales.any() and not grads[1].amplitudes.any() and grads[0].lengthscales.any()


def test_sample_opt_map(B):
    prob = _problem(B, kernel_of(B, "expo", 2))
    scored = B.HipBatchedMAP(samples=12, seed=1).estimate_parameters(prob, return_all=True)
    top = sorted((s.loglike for s in scored), reverse=True)[:3]
    res = B.HipSampleOptMAP(12, 3, 4, seed=1).estimate_parameters(prob, return_all=True)
    ends = sorted((r.loglike for r in res), reverse=True)
    print(f"[kgrad] HipSampleOptMAP: best three samples {top} -> {ends}")
    assert len(res) == 3 and all(e >= t for e, t in zip(ends, top))


def test_gradient_am_returns_an_in_domain_point_no_worse_than_its_starts(B, api):
    from boss_jl_amd.bo import estimate_parameters
    prob = _problem(B, kernel_of(B, "expo", 2))
    estimate_parameters(prob, B.HipBatchedMAP(samples=16, seed=1))
    x_prior = lambda r: r.uniform(0, 1, 2)
    am = B.HipGradientAM(x_prior=x_prior, multistart=8, iters=5, seed=3)
    x, val = am.maximize_acquisition(prob)
    assert x.shape == (2,) and np.all((x >= 0.0) & (x <= 1.0)) and np.isfinite(val)
    # the starts it drew (iters = 0 returns the best of them)
    x0, val0 = B.HipGradientAM(x_prior=x_prior, multistart=8, iters=0, seed=3).maximize_acquisition(prob)
    print(f"[kgrad] HipGradientAM: best start {val0:.6e} -> {val:.6e}")
    assert val >= val0
    # mean_and_var_grad of the model's posterior, slices and all outputs
    post = prob.model.model_posterior(prob.params, prob.data)
    try:
        X = np.stack([x, x0], axis=1)
        mu, var, dmu, dvar = post.slices[0].mean_and_var_grad(X)
        allp = post.mean_and_var_grad(X)
        assert np.array_equal(allp[0][0], mu) and np.array_equal(allp[3][0], dvar) and dmu.shape == (2, 2)
        m0, v0 = post.slices[0].mean_and_var(X)
        assert np.abs(m0 - mu).max() <= 1e-9 * (1 + np.abs(mu).max()) and np.abs(v0 - var).max() <= 1e-9
    finally:
        post.close()
