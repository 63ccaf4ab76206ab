"""Program-kernel posteriors on the device (boss_kgp_create, B.DeviceKernel): update, prediction on every finish path, acquisition,
the Python surface, and every refusal.

Expected values: the test's own numpy/scipy restatement (kernel_program_cases.Restated) — K from the Python closure with the
conventions of include/bosship.h, scipy.linalg.cholesky, then solves.  Tolerance: the project's own (tol_for, tests/test_gpu_parity.py),
tol = max(1e-9, cond(K)·N·2⁻⁵³·8), applied as there: |Δlogpdf| <= tol(1+|logpdf|), |Δμ| <= tol(1+max|μ|), |Δσ²| <= tol·max k(x*,x*).
Every input keeps cond(K) below 1e6 (asserted).

Shapes, the smallest at which each piece can go wrong:
  n20     N = 20,   d = 1,  M = 5      below SMALL_MAX_N: must not take the one-launch path of the built-in kernels
  n130    N = 130,  d = 3,  M = 70     diagonal, off-diagonal and ragged Gram tiles; predict_kernel<G32, true>; ragged candidate tile
  n130dm  the same with one discrete dimension and a prior mean
  n130w   N = 130,  d = 16, M = 33     32 inputs
  n130b   N = 130,  d = 3,  M = 16389  64-wide slabs (predict_kernel<G64, true>)
  n1030   N = 1030, d = 3,  M = 40     Np >= 1024: the few-candidates route; repeated calls reach the resident-inverse finishes"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_program_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {
    "n20": dict(d=1, N=20, M=5),
    "n130": dict(d=3, N=130, M=70),
    "n130dm": dict(d=3, N=130, M=70, discrete=[False, True, False], scale=[1.0, 4.0, 1.0], mean=True),
    "n130w": dict(d=16, N=130, M=33),
    "n130b": dict(d=3, N=130, M=16389),
    "n1030": dict(d=3, N=1030, M=40),
}
AMP = 1.0
NAMES = sorted(cases.CLOSURES)


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


def kernel_of(B, name, d):
    if (name, d) not in _kernels:
        f = cases.CLOSURES.get(name) or cases.BUILTIN[name]
        _kernels[(name, d)] = B.DeviceKernel(f, d)
    return _kernels[(name, d)]


def setup(shape, name):
    """(X, y, Xs, lam, sig, discrete, mean_X, mean_Xs, restatement) of one case, computed once and shared."""
    key = (shape, name)
    if key not in _refs:
        s = SHAPES[shape]
        d, sc = s["d"], np.asarray(s.get("scale", np.ones(s["d"])), float)
        X, y, Xs = cases.data(d, s["N"], s["M"], seed=3, scale=sc)
        lam = np.linspace(0.4, 0.6, d) * sc
        mX = 0.5 + 0.2 * X.sum(0) if s.get("mean") else None
        mXs = 0.5 + 0.2 * Xs.sum(0) if s.get("mean") else None
        f = cases.CLOSURES.get(name) or cases.BUILTIN[name]
        ref = cases.Restated(f, X, y, lam, AMP, noise_of(name), Xs, s.get("discrete"), mX, mXs)
        for a in (X, y, Xs, ref.mu, ref.var, ref.kss):
            a.setflags(write=False)
        _refs[key] = (X, y, Xs, lam, noise_of(name), s.get("discrete"), mX, mXs, ref)
    return _refs[key]


def clipped(var):
    return np.where((var < 0.0) & (var >= -1e-8), 0.0, var)


def check(tag, ref, lp, mu, var, mu_ref=None, var_ref=None, kss=None):
    mu_ref = ref.mu if mu_ref is None else mu_ref
    var_ref = ref.var if var_ref is None else var_ref
    kss = ref.kss if kss is None else kss
    tol = ref.tol
    e_mu, e_var = np.abs(mu - mu_ref).max(), np.abs(var - clipped(var_ref)).max()
    line = f"[kprog] {tag}: cond {ref.cond:.3e} tol {tol:.3e}"
    if lp is not None:
        line += f" |dlogpdf| {abs(lp - ref.logpdf):.3e} (bound {tol * (1 + abs(ref.logpdf)):.3e})"
    print(line + f" |dmu| {e_mu:.3e} (bound {tol * (1 + np.abs(mu_ref).max()):.3e}) |dvar| {e_var:.3e} (bound {tol * kss.max():.3e})")
    assert ref.cond < 1e6
    if lp is not None:
        assert abs(lp - ref.logpdf) <= tol * (1 + abs(ref.logpdf))
    assert e_mu <= tol * (1 + np.abs(mu_ref).max())
    assert e_var <= tol * kss.max()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", ["n20", "n130", "n130dm", "n130w", "n130b"])
def test_update_and_predict_match_the_restatement(B, api, shape, name):
    X, y, Xs, lam, sig, disc, mX, mXs, ref = setup(shape, name)
    g = api.KernelGP(X, y, kernel_of(B, name, X.shape[0]).program, disc)
    try:
        lp = g.update(lam, AMP, sig, mX)
        mu, var = g.predict(Xs, mXs)
        check(f"{shape} {name}", ref, lp, mu, var)
        if name == "dot1":
            assert np.ptp(ref.kss) > 0.1 * ref.kss.max()     # the prior variance differs from candidate to candidate
        mu2, var2 = g.predict(Xs, mXs)                       # no atomics: repeated calls agree bit for bit
        assert np.array_equal(mu, mu2) and np.array_equal(var, var2)
        assert g.update(lam, AMP, sig, mX) == lp
    finally:
        g.close()


@pytest.mark.parametrize("name", NAMES)
def test_few_candidates_route_and_its_resident_inverse_finishes(B, api, name):
    """N = 1030 (Np = 1280): the step path first, then — from the winv_after()-th call on one factorisation — the one-pass finish
    over L⁻ᵀ for M <= 4 (winv_finish_kernel) and the inverse GEMMs above that (inv_fwd_finish_kernel).  The route is read from the
    handle (boss_debug_acq_counters: its few-candidates call count and whether the inverse factors are resident); with them resident
    predict_enqueue takes use_winv for M <= 4 and use_invgemm for up to invgemm_max_tiles() tiles of 32, so the knobs that would
    send the calls elsewhere must be at their defaults."""
    for knob in ("BOSS_INVGEMM_MAX_TILES", "BOSS_FEW_MAX_TILES", "BOSS_NO_FEW"):
        assert os.environ.get(knob) is None, knob + " is set: this test would not reach the resident-inverse finishes"
    winv_after = int(os.environ.get("BOSS_WINV_AFTER", "2"))   # (winv_after(), host_append.inc)
    assert winv_after >= 1, "BOSS_WINV_AFTER=0 switches the resident inverses off"
    X, y, Xs, lam, sig, disc, mX, mXs, ref = setup("n1030", name)
    g = api.KernelGP(X, y, kernel_of(B, name, 3).program)
    try:
        for M in (40, 3):
            lp = g.update(lam, AMP, sig)                     # a new factorisation: the call count starts over
            assert api._acq_counters(g)[:2] == (0, 0)
            for rep in range(winv_after + 2):
                mu, var = g.predict(Xs[:, :M])
                have_winv, few_calls = api._acq_counters(g)[:2]
                # calls 1 .. winv_after - 1 take the step path; call winv_after builds L⁻ᵀ, L⁻¹ and finishes on them, as do all later ones
                assert have_winv == (1 if rep + 1 >= winv_after else 0) and few_calls == min(rep + 1, winv_after), (rep, have_winv, few_calls)
                check(f"n1030 {name} M={M} call {rep}", ref, lp if rep == 0 else None, mu, var, ref.mu[:M], ref.var[:M], ref.kss[:M])
    finally:
        g.close()


@pytest.mark.parametrize("kernel", sorted(cases.BUILTIN))
def test_agrees_with_the_built_in_kernel_and_the_oracle(B, api, O, kernel):
    X, y, Xs, lam, sig, _, _, _, ref = setup("n130", kernel)
    post = O.gp_fit(X, y, kernel, lam, AMP, sig)
    mu_o, var_o = O.gp_mean_and_var(post, Xs, clip=False)
    gk = api.KernelGP(X, y, kernel_of(B, kernel, 3).program)
    gb = api.GP(X, y, kernel)
    try:
        lp_k, lp_b = gk.update(lam, AMP, sig), gb.update(lam, AMP, sig)
        (mu_k, var_k), (mu_b, var_b) = gk.predict(Xs), gb.predict(Xs)
        tol = ref.tol
        print(f"[kprog] builtin {kernel}: tol {tol:.3e} vs handle: dlogpdf {abs(lp_k - lp_b):.3e} dmu {np.abs(mu_k - mu_b).max():.3e} "
              f"dvar {np.abs(var_k - var_b).max():.3e}; vs oracle: dlogpdf {abs(lp_k - post.logpdf):.3e} dmu {np.abs(mu_k - mu_o).max():.3e} "
              f"dvar {np.abs(var_k - clipped(var_o)).max():.3e}")
        assert ref.cond < 1e6
        for lp, mu, var in ((lp_b, mu_b, var_b), (post.logpdf, mu_o, clipped(var_o))):
            assert abs(lp_k - lp) <= tol * (1 + abs(lp))
            assert np.abs(mu_k - mu).max() <= tol * (1 + np.abs(mu).max())
            assert np.abs(var_k - var).max() <= tol * ref.kss.max()
    finally:
        gk.close()
        gb.close()


def test_acq_ei_over_outputs_and_samples(B, api, O, monkeypatch):
    """boss_acq_ei with P = 2 (y_max = [inf, 0.5]) and S = 3 program handles against oracle.gp_oracle.ei_acquisition evaluated on the
    restatement's moments.  Bound on the acquisition: with s the smallest posterior standard deviation over all handles and
    candidates, tol_μ = tol(1+max|μ|), tol_v = tol·max k(x*,x*), E = EI of output 0 (coefficient 1), F = Φ((y_max − μ₁)/σ₁):
        |ΔE| <= tol_μ + 0.4·tol_v/(2s)        (∂EI/∂μ = Φ <= 1, ∂EI/∂σ = φ <= 0.4, Δσ <= Δσ²/(2σ))
        |ΔF| <= 0.4·tol_μ/s + 0.242·tol_v/(2s²)   (φ <= 0.4, |z|φ(z) <= 0.242)
        |Δacq| <= |ΔE| + max E · |ΔF|, the mean over samples no larger."""
    d, N, M, P, S = 3, 130, 70, 2, 3
    X, y0, Xs = cases.data(d, N, M, seed=5)
    Y = np.stack([y0, 0.4 + 0.3 * np.cos(3.0 * X.sum(0))])
    names = ["expo", "dot1"]
    gps, refs = [], []
    try:
        for s in range(S):
            row, rrow = [], []
            for p in range(P):
                lam = np.linspace(0.4, 0.6, d) * (1.0 + 0.15 * s)
                sig = noise_of(names[p]) * (1.0 + 0.2 * s)
                g = api.KernelGP(X, Y[p], kernel_of(B, names[p], d).program)
                row.append(g)
                g.update(lam, AMP, sig)
                rrow.append(cases.Restated(cases.CLOSURES[names[p]], X, Y[p], lam, AMP, sig, Xs))
            gps.append(row)
            refs.append(rrow)
        coefs, y_max = [1.0, 0.0], [np.inf, 0.5]
        best = O.best_so_far(coefs, Y, y_max)
        assert best is not None
        cand = api.Candidates(Xs)
        acq, am, mx = api.acq_ei(gps, cand, coefs, y_max, best)
        _, am2, mx2 = api.acq_ei(gps, cand, coefs, y_max, best, want_acq=False)
        cand.close()
        moments = {s: (np.stack([r.mu for r in refs[s]]), np.stack([clipped(r.var) for r in refs[s]])) for s in range(S)}
        monkeypatch.setattr(O, "model_mean_and_var", lambda posts, Xs_, means_s=None: moments[posts[0]])
        want = O.ei_acquisition([[s] for s in range(S)], Xs, coefs, y_max, best)
        allr = [r for row in refs for r in row]
        tol = max(r.tol for r in allr)
        assert max(r.cond for r in allr) < 1e6
        smin = min(np.sqrt(np.maximum(r.var, 0.0)).min() for r in allr)
        tol_mu = tol * (1 + max(np.abs(r.mu).max() for r in allr))
        tol_v = tol * max(r.kss.max() for r in allr)
        e_max = max(O.expected_improvement_lin(coefs, *moments[s], best).max() for s in range(S))
        bound = tol_mu + 0.4 * tol_v / (2 * smin) + e_max * (0.4 * tol_mu / smin + 0.242 * tol_v / (2 * smin * smin))
        print(f"[kprog] acq P=2 S=3: max|dacq| {np.abs(acq - want).max():.3e} (bound {bound:.3e}, smin {smin:.3e}), argmax {am} / {int(np.argmax(want))}")
        assert np.abs(acq - want).max() <= bound
        assert am == int(np.argmax(want)) and am2 == am and mx2 == mx and mx == acq[am]
    finally:
        for row in gps:
            for g in row:
                g.close()


def _problem(B, dk, X, Y, seed):
    pri = dict(lengthscale_priors=[B.MvLogNormal(np.log([0.5, 0.5]), [0.2, 0.2])], amplitude_priors=[B.LogNormal(0.0, 0.2)],
               noise_std_priors=[B.Dirac(0.05)])
    model = B.HipGaussianProcess(kernel=dk, **pri)
    f = lambda x: [np.sin(3.0 * x[0]) + np.cos(2.0 * x[1])]
    return B.BossProblem(f, B.Domain(([0.0, 0.0], [1.0, 1.0])), B.ExpectedImprovement(B.LinFitness([1.0])), model,
                         B.ExperimentData(X, Y))


def test_python_surface_bo_steps_and_moments(B, api):
    """Two bo_steps with HipBatchedMAP + HipBatchAM on an exponential-kernel model, the maximiser's return_all values against the
    restatement, and the model's posterior / likelihood calls against each other."""
    from boss_jl_amd.bo import bo_step, estimate_parameters
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (2, 24))
    Y = (np.sin(3.0 * X[0]) + np.cos(2.0 * X[1]))[None, :]
    dk = kernel_of(B, "expo", 2)
    prob = _problem(B, dk, X, Y, 0)
    fitter = B.HipBatchedMAP(samples=16, seed=1)
    am = B.HipBatchAM(x_prior=lambda r: r.uniform(0, 1, 2), samples=300, seed=2)
    assert am.fused and not am._fusable(prob)                 # the default fused=True takes the two-call path silently
    for _ in range(2):
        x, val = bo_step(prob, fitter, am)
        assert x.shape == (2,) and np.all((x >= 0.0) & (x <= 1.0)) and np.isfinite(val)
        prob.consistent = False
    assert prob.data.X.shape[1] == 26
    estimate_parameters(prob, fitter)
    Xs, acq = am.maximize_acquisition(prob, return_all=True)
    prm = prob.params
    ref = cases.Restated(cases.expo, prob.data.X, prob.data.Y[0], prm.lengthscales[:, 0], prm.amplitudes[0], prm.noise_std[0], Xs)
    from oracle import gp_oracle as O
    best = O.best_so_far([1.0], prob.data.Y, [np.inf])
    want = O.expected_improvement_lin([1.0], ref.mu[None, :], clipped(ref.var)[None, :], best)
    smin = np.sqrt(np.maximum(ref.var, 0.0)).min()
    bound = ref.tol * (1 + np.abs(ref.mu).max()) + 0.4 * ref.tol * ref.kss.max() / (2 * smin)
    print(f"[kprog] bo return_all: max|dacq| {np.abs(acq - want).max():.3e} (bound {bound:.3e}), cond {ref.cond:.3e}")
    assert ref.cond < 1e6 and np.abs(acq - want).max() <= bound
    # posterior: one parameter set and a list of samples; mean / var / std / mean_and_var; average_mean
    model = prob.model
    post = model.model_posterior(prm, prob.data)
    samples = [prm, B.HipGPParams(prm.lengthscales * 1.1, prm.amplitudes, prm.noise_std)]
    posts = model.model_posterior(samples, prob.data)
    try:
        mu, var = post.mean_and_var(Xs[:, :9])
        check("python posterior", ref, None, mu[0], var[0], ref.mu[:9], ref.var[:9], ref.kss[:9])
        assert np.array_equal(post.mean(Xs[:, :9]), mu) and np.array_equal(post.var(Xs[:, :9]), var)
        assert np.allclose(post.std(Xs[:, :9]), np.sqrt(var), rtol=0, atol=0)
        m1, v1 = post.slices[0].mean_and_var(Xs[:, 0])
        assert abs(m1 - ref.mu[0]) <= ref.tol * (1 + abs(ref.mu[0])) and abs(v1 - clipped(ref.var)[0]) <= ref.tol * ref.kss.max()
        assert np.array_equal(posts[0].mean(Xs[:, :9]), mu)
        avg = B.average_mean(posts, Xs[:, :9])
        assert np.array_equal(avg, (posts[0].mean(Xs[:, :9]) + posts[1].mean(Xs[:, :9])) / 2)
        # likelihoods: data_loglike, data_loglike_batch (S updates on one handle), params_loglike / sampler
        ll = model.data_loglike(prob.data)
        one = ll(prm)
        assert abs(one - ref.logpdf) <= ref.tol * (1 + abs(ref.logpdf))
        batch = model.data_loglike_batch(prob.data, samples)
        assert batch[0] == one and batch[1] == ll(samples[1])
        # an invalid parameter set is a sample of likelihood -inf, as in the batched call of the built-in kernels
        bad = B.HipGPParams(prm.lengthscales, -prm.amplitudes, prm.noise_std)
        b3 = model.data_loglike_batch(prob.data, [prm, bad, samples[1]])
        assert b3[0] == one and b3[1] == -np.inf and b3[2] == batch[1]
        for h in ll.handles:
            h.close()
        assert np.isfinite(model.params_loglike()(model.params_sampler()(np.random.default_rng(0))))
        # refusals of the Python surface, each naming DeviceKernel
        sl = post.slices[0]
        for call in (lambda: sl.mean_and_var_grad(Xs[:, :3]), lambda: sl.mean_and_cov(Xs[:, :3]), lambda: post.cov(Xs[:, :3]),
                     lambda: sl.append(Xs[:, 0], 0.0), lambda: post.append(Xs[:, 0], [0.0]),
                     lambda: B.HipGradientMAP(2, 2, seed=0).estimate_parameters(prob),
                     lambda: B.HipSampleOptMAP(4, 2, 2, seed=0).estimate_parameters(prob),
                     lambda: B.HipGradientAM(x_prior=lambda r: r.uniform(0, 1, 2), multistart=4, iters=2, seed=0).maximize_acquisition(prob),
                     lambda: B.HipSequentialBatchAM(am, 2).maximize_acquisition(prob),
                     lambda: B.HipBatchAM(points=Xs[:, :8], devices=[0]).maximize_acquisition(prob),
                     lambda: model.data_loglike_grad_batch(prob.data, samples)):
            with pytest.raises(NotImplementedError, match="DeviceKernel"):
                call()
        # the shard modes of one process run on moments: the same epilogue on the same moments, so the same values
        _, acq_o = B.HipBatchAM(points=Xs, shard="outputs").maximize_acquisition(prob, return_all=True)
        assert np.array_equal(acq_o, acq)
        prob.params = samples                                # (shard="samples" splits a list of parameter samples)
        _, acq_c = B.HipBatchAM(points=Xs).maximize_acquisition(prob, return_all=True)
        _, acq_s = B.HipBatchAM(points=Xs, shard="samples").maximize_acquisition(prob, return_all=True)
        _, acq_so = B.HipBatchAM(points=Xs, shard="outputs").maximize_acquisition(prob, return_all=True)
        assert np.array_equal(acq_s, acq_c)
        assert np.abs(acq_so - acq_c).max() <= 2 * np.finfo(float).eps * np.abs(acq_c).max()   # (the mean over two samples, taken by another kernel)
        prob.params = prm
    finally:
        post.close()
        for p in posts:
            p.close()


def test_not_positive_definite(B, api):
    X = np.array([[0.1, 0.1, 0.7, 0.4]])                     # a duplicated point, σ = 0
    g = api.KernelGP(X, np.array([0.0, 1.0, 0.5, 0.2]), kernel_of(B, "dot1", 1).program)
    try:
        with pytest.raises(api.PosDefException):
            g.update([0.5], 1.0, 0.0)
        with pytest.raises(api.BossError) as e:
            g.predict(X)
        assert e.value.code == api.BOSS_E_NOT_FITTED
        assert np.isfinite(g.update([0.5], 1.0, 0.3))         # the handle stays usable
    finally:
        g.close()


def test_refused_entry_points_and_the_built_in_handle_next_to_it(B, api):
    """Every entry point that takes a boss_gp_t* but no program-kernel posterior returns BOSS_E_INVALID and says so; a built-in
    handle on the same context gives the same arrays before and after the program handle's calls."""
    X, y, Xs, lam, sig, _, _, _, ref = setup("n130", "expo")
    gb = api.GP(X, y, "matern52")
    lp_b = gb.update(lam, AMP, sig)
    before = gb.predict(Xs)
    cand = api.Candidates(Xs)
    acq_before = api.acq_ei([[gb]], cand, [1.0], None, float(y.max()))
    g = api.KernelGP(X, y, kernel_of(B, "expo", 3).program)
    lib = api.load_library()
    try:
        g.update(lam, AMP, sig)
        mu, var = g.predict(Xs)
        fit = B.DeviceFitness(lambda yv: yv[0] * yv[0], 1).program
        eps = np.random.default_rng(0).standard_normal((1, 8))
        warp = api.WarpProgram(B.trace_mean(lambda x: [x[0], x[1], x[2]], 3, 0, 3), 1, None)
        assert api.init() >= 1                               # the one-process multi-device calls: G = 1 on the device boss_init opened
        mcand = api.MultiCandidates(Xs[:, :9], 1)
        Xb, yb = setup("n1030", "expo")[:2]                  # ten block columns: a step k = 2 exists for the rider's timing aid
        gbig = api.KernelGP(Xb, yb, kernel_of(B, "expo", 3).program)
        replay = lib.boss_debug_rider_replay
        replay.restype = C.c_int
        replay.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        refused = {
            "boss_gp_update_acq": lambda: g.update_acq(lam, AMP, sig, cand),
            "boss_gp_append": lambda: g.append(Xs[:, 0], 0.0),
            "boss_gp_reserve": lambda: g.reserve(200),
            "boss_track_create": lambda: api.Track(g, cand),
            "boss_gp_predict_grad": lambda: g.predict_grad(Xs[:, :3]),
            "boss_acq_ei_grad": lambda: api.acq_ei_grad([g], Xs[:, :3], [1.0], None, 0.0),
            "boss_acq_ei_grad_set": lambda: api.acq_ei_grad_set([[g], [g]], Xs[:, :3], [1.0], None, 0.0),
            "boss_gp_loglike_grad": lambda: g.loglike_grad(),
            "boss_gp_loglike_grad_mean": lambda: g.loglike_grad_mean(),
            "boss_gp_predict_cov": lambda: g.predict_cov(Xs[:, :3]),
            "boss_warp_predict": lambda: warp.predict([[g]], Xs[:, :3]),
            "boss_warp_predict_grad": lambda: warp.predict_grad([[g]], Xs[:, :3]),
            "boss_acq_ei_warp": lambda: warp.acq_ei([[g]], Xs[:, :3], [1.0], None, 0.0),
            "boss_acq_ei_grad_warp": lambda: warp.acq_ei_grad([[g]], Xs[:, :3], [1.0], None, 0.0),
            "boss_acq_ei_mc": lambda: api.acq_ei_mc([[g]], cand, fit, eps, None, 0.0),
            "boss_acq_ei_mc_grad": lambda: api.acq_ei_mc_grad([[g]], Xs[:, :3], fit, eps, None, 0.0),
            "boss_multi_gp_update": lambda: api.multi_update([g], lam, AMP, sig),
            "boss_multi_acq_ei": lambda: api.multi_acq_ei([[[g]]], Xs[:, :9], [1.0], None, 0.0),
            "boss_multi_acq_ei_cand": lambda: api.multi_acq_ei_cand([[[g]]], mcand, [1.0], None, 0.0),
            "boss_multi_acq_ei_outputs": lambda: api.multi_acq_ei_outputs([[g]], Xs[:, :9], [1.0], None, 0.0),
            "boss_multi_acq_ei_samples": lambda: api.multi_acq_ei_samples([[g]], Xs[:, :9], [1.0], None, 0.0),
            "boss_debug_rider_replay": lambda: api._check(replay(gbig._h, cand._h, 2, 1, 0, C.byref(C.c_double(0.0)))),
            "boss_nlat_create": lambda: api.NgpLatents([(g, ("none", (0.0, 0.0), "identity", 0.0)), 0.5, 0.5], 1.0),
        }
        for name, call in refused.items():
            with pytest.raises(api.BossError) as e:
                call()
            assert e.value.code == api.BOSS_E_INVALID and "program-kernel posteriors" in str(e.value), (name, str(e.value))
        # the other models' own entry points refuse a handle they did not create
        lam_c = api._f64(np.asarray(lam, float), 1)
        for call in (lambda: lib.boss_ngp_reserve(g._h, 200), lambda: lib.boss_ggp_reserve(g._h, 200),
                     lambda: lib.boss_ggp_update(g._h, api._dp(lam_c), AMP, sig, 0.1, 0, None)):
            assert call() == api.BOSS_E_INVALID and "was not created by" in lib.boss_last_error().decode()
        warp.close()
        mcand.close()
        gbig.close()
        # nothing of the refusals disturbed the program handle, and the built-in handle computes what it computed before
        mu2, var2 = g.predict(Xs)
        assert np.array_equal(mu, mu2) and np.array_equal(var, var2)
        after = gb.predict(Xs)
        acq_after = api.acq_ei([[gb]], cand, [1.0], None, float(y.max()))
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert np.array_equal(acq_before[0], acq_after[0]) and acq_before[1:] == acq_after[1:]
        assert gb.update(lam, AMP, sig) == lp_b
        # a mixed call: built-in and program handles side by side go member by member
        acq_mix, am_mix, _ = api.acq_ei([[gb, g]], cand, [1.0, 0.0], [np.inf, 0.5], float(y.max()))
        acq_solo, am_solo, _ = api.acq_ei([[gb]], cand, [1.0], [np.inf], float(y.max()))
        assert acq_mix.shape == acq_solo.shape and np.all(acq_mix <= acq_solo)
    finally:
        cand.close()
        g.close()
        gb.close()
