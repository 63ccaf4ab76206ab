"""Derivatives of kernel programs without a device: the reverse sweep behind a traced kernel (boss_kern_grad_host,
api.KernelProgram.grad) against closed forms, its convention at coincident points, the unchanged sweep of fitness programs, the
grad=True validation of B.DeviceKernel, and the numpy/scipy restatement the GPU tests take their expected gradients from
(kernel_grad_cases.RestatedGrad) against central differences of itself and against the oracle on the built-in kernels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_program_cases as cases  # noqa: E402
import kernel_grad_cases as gcases  # noqa: E402

NAMES = sorted(gcases.ALL)


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


@pytest.mark.parametrize("name", NAMES)
def test_closed_forms_agree_with_central_differences_of_the_closures(name):
    """h = 1e-5: truncation ~ h²·|f'''| <= 1e-9, rounding ~ ε/h ~ 1e-11 — held to 1e-7·max(1, |∂f|)."""
    f = gcases.ALL[name]
    rng = np.random.default_rng(7)
    U, V = rng.standard_normal((3, 50)), rng.standard_normal((3, 50))
    gu, gv = gcases.PARTIALS[name](U, V)
    fu, fv = gcases.fd_partials(f, U, V)
    err = max(np.abs(gu - fu).max(), np.abs(gv - fv).max())
    print(f"[kgrad-host] {name}: max|closed form - central difference| {err:.3e}")
    assert np.all(np.abs(gu - fu) <= 1e-7 * np.maximum(1.0, np.abs(gu))) and np.all(np.abs(gv - fv) <= 1e-7 * np.maximum(1.0, np.abs(gv)))


@pytest.mark.parametrize("d", [1, 3, 16])
@pytest.mark.parametrize("name", NAMES)
def test_the_sweep_matches_the_closed_forms(B, api, name, d):
    prog = B.DeviceKernel(gcases.ALL[name], d).program       # (grad=False: the sweep itself needs no switch)
    rng = np.random.default_rng(200 + d)
    U, V = rng.standard_normal((d, 100)), rng.standard_normal((d, 100))
    gu, gv = gcases.PARTIALS[name](U, V)
    k, dU, dV = prog.grad(U, V)
    # the C entry point itself, k_out NULL
    Uf, Vf = np.asfortranarray(U), np.asfortranarray(V)
    cU, cV = np.zeros((d, 100), order="F"), np.zeros((d, 100), order="F")
    assert api.load_library().boss_kern_grad_host(prog._h, 100, api._dp(Uf), api._dp(Vf), None, api._dp(cU), api._dp(cV)) == api.BOSS_OK
    assert np.array_equal(cU, dU) and np.array_equal(cV, dV) and np.array_equal(k, prog.eval_host(U, V))
    err = max(np.abs(dU - gu).max(), np.abs(dV - gv).max())
    print(f"[kgrad-host] {name} d={d}: max|sweep - closed form| {err:.3e}")
    assert np.all(np.abs(dU - gu) <= 1e-12 * np.maximum(1.0, np.abs(gu))) and np.all(np.abs(dV - gv) <= 1e-12 * np.maximum(1.0, np.abs(gv)))
    k1, u1, v1 = prog.grad(U[:, 0], V[:, 0])                 # one point pair
    assert k1 == k[0] and np.array_equal(u1, dU[:, 0]) and np.array_equal(v1, dV[:, 0])


@pytest.mark.parametrize("d", [1, 3, 16])
@pytest.mark.parametrize("name", NAMES)
def test_coincident_pairs_are_finite_and_zero_for_stationary_kernels(B, name, d):
    prog = B.DeviceKernel(gcases.ALL[name], d).program
    U = np.random.default_rng(300 + d).standard_normal((d, 20))
    _, dU, dV = prog.grad(U, U)
    assert np.all(np.isfinite(dU)) and np.all(np.isfinite(dV))
    if name in gcases.STATIONARY:
        assert not dU.any() and not dV.any()
    else:                                                    # dot1: ∂/∂u (u·v + 1) = v
        assert np.allclose(dU, U, rtol=0, atol=1e-15) and np.allclose(dV, U, rtol=0, atol=1e-15)


def test_bad_arguments_of_the_c_entry_point(B, api):
    lib = api.load_library()
    prog = B.DeviceKernel(cases.expo, 2).program
    z = np.zeros(2)
    assert lib.boss_kern_grad_host(None, 1, api._dp(z), api._dp(z), None, api._dp(z), api._dp(z)) == api.BOSS_E_INVALID
    assert lib.boss_kern_grad_host(prog._h, 1, api._dp(z), api._dp(z), None, None, api._dp(z)) == api.BOSS_E_INVALID
    assert lib.boss_kern_grad_host(prog._h, 0, None, None, None, None, None) == api.BOSS_OK
    assert lib.boss_kgp_set_grad(None, 1) == api.BOSS_E_INVALID


def test_fitness_programs_keep_their_sweep(B):
    """sqrt(y²) at y = 0: a fitness program's reverse sweep still multiplies SQRT'(0) = +Inf by SQUARE' = 0 (NaN), through the host
    entry the kernels share; the same spelling as a kernel program gives 0."""
    fit = B.DeviceFitness(lambda y: np.sqrt(y[0] * y[0]) + y[1], 2).program
    f, df = fit.eval_host(np.array([[0.0, 2.0], [0.5, 0.5]]), want_grad=True)
    assert np.array_equal(f, [0.5, 2.5])
    assert np.isnan(df[0, 0]) and df[1, 0] == 1.0 and df[0, 1] == 1.0 and df[1, 1] == 1.0
    ref = fit.grad(np.array([[0.0, 2.0], [0.5, 0.5]]))       # the numpy interpreter of the same conventions
    assert np.array_equal(np.isnan(ref), np.isnan(df)) and np.array_equal(ref[~np.isnan(ref)], df[~np.isnan(df)])
    kern = B.DeviceKernel(lambda u, v: np.sqrt((u[0] - v[0]) * (u[0] - v[0])) + 1.0, 1).program
    _, du, dv = kern.grad(np.array([0.3]), np.array([0.3]))
    assert du[0] == 0.0 and dv[0] == 0.0


def _problem_data(d=3, N=40, M=9, seed=2):
    X, y, Xs = cases.data(d, N, M, seed=seed)
    return X, y, Xs, np.linspace(0.4, 0.6, d)


@pytest.mark.parametrize("name", NAMES)
def test_restated_likelihood_gradient_matches_differences_of_its_own_logpdf(name):
    """Central differences of logpdf with h = 1e-6, one discrete dimension and a prior mean.  Truncation (h²) is negligible; each logpdf
    carries about 1e-13·(1 + |logpdf|) of rounding (N = 40, |logpdf| ~ 1e2), which over 2h is ~1e-5 absolute at worst: held to
    1e-5·(1 + max|grad|)."""
    f = gcases.ALL[name]
    X, y, Xs, lam = _problem_data()
    amp, sig = 1.1, 0.1 if name == "dot1" else 0.05
    mX = 0.1 * X.sum(0)
    disc = [False, True, False]
    Xd = X * np.array([1.0, 4.0, 1.0])[:, None]
    lamd = lam * np.array([1.0, 4.0, 1.0])
    ref = gcases.RestatedGrad(f, Xd, y, lamd, amp, sig, None, disc, mX, want_cond=False)
    h = 1e-6
    fd = np.zeros(5)
    for q in range(5):
        vals = []
        for sgn in (1.0, -1.0):
            l2, a2, s2 = lamd.copy(), amp, sig
            if q < 3:
                l2[q] += sgn * h
            elif q == 3:
                a2 += sgn * h
            else:
                s2 += sgn * h
            vals.append(cases.Restated(f, Xd, y, l2, a2, s2, None, disc, mX, want_cond=False).logpdf)
        fd[q] = (vals[0] - vals[1]) / (2 * h)
    err = np.abs(ref.dlogpdf - fd).max()
    print(f"[kgrad-host] {name}: max|dlogpdf - differences| {err:.3e} (max|grad| {np.abs(fd).max():.3e})")
    assert err <= 1e-5 * (1 + np.abs(fd).max())


@pytest.mark.parametrize("name", NAMES)
def test_restated_moment_gradients_match_differences_of_predict(name):
    """Central differences of `predict` with h = 1e-6 (μ, σ² of order 1 with ~1e-13 of rounding: ~1e-7 over 2h), a prior mean with
    gradient 0.2 in every dimension: held to 1e-6·(1 + max|gradient|); then a discrete dimension."""
    f = gcases.ALL[name]
    X, y, Xs, lam = _problem_data()
    sig = 0.1 if name == "dot1" else 0.05
    mg = np.full((3, Xs.shape[1]), 0.2)
    ref = gcases.RestatedGrad(f, X, y, lam, 1.1, sig, Xs, None, 0.2 * X.sum(0), 0.2 * Xs.sum(0), mg, want_cond=False)
    h = 1e-6
    for m in range(3):
        Xp, Xm = Xs.copy(), Xs.copy()
        Xp[m] += h
        Xm[m] -= h
        mp, vp, _ = ref.predict(Xp, 0.2 * Xp.sum(0))
        mm, vm, _ = ref.predict(Xm, 0.2 * Xm.sum(0))
        e_mu, e_var = np.abs((mp - mm) / (2 * h) - ref.dmu[m]).max(), np.abs((vp - vm) / (2 * h) - ref.dvar[m]).max()
        print(f"[kgrad-host] {name} dim {m}: |dmu - differences| {e_mu:.3e} |dvar - differences| {e_var:.3e}")
        assert e_mu <= 1e-6 * (1 + np.abs(ref.dmu).max()) and e_var <= 1e-6 * (1 + np.abs(ref.dvar).max())
    # a discrete dimension: the kernel parts vanish, the prior mean's own gradient stays
    disc = [False, True, False]
    refd = gcases.RestatedGrad(f, X, y, lam, 1.1, sig, Xs, disc, None, None, mg, want_cond=False)
    assert np.array_equal(refd.dmu[1], mg[1]) and not refd.dvar[1].any()


@pytest.mark.parametrize("kernel", sorted(cases.BUILTIN))
def test_restatement_agrees_with_the_oracle_on_built_in_kernels(O, kernel):
    X, y, Xs, lam = _problem_data()
    ref = gcases.RestatedGrad(cases.BUILTIN[kernel], X, y, lam, 1.1, 0.05, Xs)
    lp, grad = O.gp_data_loglike_grad(X, y, kernel, lam, 1.1, 0.05)
    post = O.gp_fit(X, y, kernel, lam, 1.1, 0.05)
    mu, var, dmu, dvar = O.gp_mean_and_var_grad(post, Xs)
    tol = max(1e-8, ref.tol)
    print(f"[kgrad-host] oracle {kernel}: dlogpdf {np.abs(grad - ref.dlogpdf).max():.3e} dmu {np.abs(dmu - ref.dmu).max():.3e} "
          f"dvar {np.abs(dvar - ref.dvar).max():.3e} (tol {tol:.3e})")
    assert abs(lp - ref.logpdf) <= tol * (1 + abs(lp))
    assert np.abs(grad - ref.dlogpdf).max() <= tol * (1 + np.abs(grad).max())
    assert np.abs(dmu - ref.dmu).max() <= tol * (1 + np.abs(dmu).max())
    assert np.abs(dvar - ref.dvar).max() <= tol * (1 + np.abs(dvar).max())


@pytest.mark.parametrize("name", NAMES)
def test_device_kernel_with_gradients_accepts_the_closures(B, name):
    for d in (1, 3):
        dk = B.DeviceKernel(gcases.ALL[name], d, grad=True)
        assert dk.grad and dk.program.d == d
    assert not B.DeviceKernel(gcases.ALL[name], 2).grad


def test_device_kernel_with_gradients_refuses_a_bad_derivative(B):
    """exp(-sqrt|Δ|) with |Δ| spelled by two maxima: at coincident points MAX passes SQRT'(0) = +Inf on to its first operand (partial 1,
    not 0), so the partials are not finite there — as the function's own derivative is not."""
    def f(u, v):
        return np.exp(-np.sqrt(np.maximum(u[0] - v[0], 0.0) + np.maximum(v[0] - u[0], 0.0)))
    with pytest.raises(ValueError, match="grad=True.*coincident"):
        B.DeviceKernel(f, 1, grad=True)
    B.DeviceKernel(f, 1)                                     # (accepted without gradients: only HipBatchAM-style use)


def test_without_the_switch_every_gradient_call_still_raises(B):
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (2, 12))
    Y = (np.sin(3.0 * X[0]) + np.cos(2.0 * X[1]))[None, :]
    model = B.HipGaussianProcess(kernel=B.DeviceKernel(cases.expo, 2), lengthscale_priors=[B.MvLogNormal(np.log([0.5, 0.5]), [0.2, 0.2])],
                                 amplitude_priors=[B.LogNormal(0.0, 0.2)], noise_std_priors=[B.Dirac(0.05)])
    prob = B.BossProblem(lambda x: [0.0], B.Domain(([0.0, 0.0], [1.0, 1.0])), B.ExpectedImprovement(B.LinFitness([1.0])), model,
                         B.ExperimentData(X, Y))
    prm = B.HipGPParams(np.full((2, 1), 0.5), np.array([1.0]), np.array([0.05]))
    for call in (lambda: B.HipGradientMAP(2, 2, seed=0).estimate_parameters(prob),
                 lambda: B.HipSampleOptMAP(4, 2, 2, seed=0).estimate_parameters(prob),
                 lambda: B.HipGradientAM(x_prior=lambda r: r.uniform(0, 1, 2), multistart=4, iters=2, seed=0).maximize_acquisition(prob),
                 lambda: model.data_loglike_grad_batch(prob.data, [prm])):
        with pytest.raises(NotImplementedError, match="DeviceKernel.*grad=True"):
            call()
