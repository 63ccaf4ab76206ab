"""Host-side checks of the likelihood gradient through the prior mean (no GPU): the header, the signatures and the built library's
exports, the wrapper's layout of shared and per-set Jacobians against a fake library, the model layer's sum over the outputs,
the central-difference Jacobian, the Normal prior, and the gradient fitter over a Semiparametric model."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _doubles(ptr, n):
    return None if ptr is None else np.ctypeslib.as_array(ptr, shape=(n,)).copy()


class _FakeLib:
    """Stands in for libbosship.so: copies what the wrapper passes and fills the outputs with recognisable values."""

    def __init__(self):
        self.calls = []

    def boss_gp_loglike_grad_batch_mean(self, *a):
        assert len(a) == 21
        d, N, S, T, jstride = a[2], a[3], a[9], a[13], a[15]
        sizes = {4: d * N, 5: N, 6: (N * S if a[7] else N), 10: d * S, 11: S, 12: S, 14: (N * T * S if jstride else N * T)}
        self.calls.append(tuple(_doubles(v, sizes[i]) if i in sizes and v is not None else v for i, v in enumerate(a[:16])))
        for s in range(S):
            a[16][s] = -1.0 - s
            a[20][s] = 0
            for m in range(d + 2):
                a[17][s * (d + 2) + m] = 100.0 * s + m
            if a[18] is not None:
                for j in range(N):
                    a[18][s * N + j] = 1000.0 * s + j
            if a[19] is not None:
                for t in range(T):
                    a[19][s * T + t] = 10.0 * s + t
        return 0


def test_header_signatures_and_library_agree():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bosship.h")).read(), flags=re.S)
    one = re.search(r"int\s+boss_gp_loglike_grad_mean\s*\(([^;]*?)\);", hdr, re.S)
    bat = re.search(r"int\s+boss_gp_loglike_grad_batch_mean\s*\(([^;]*?)\);", hdr, re.S)
    assert one and bat
    assert one.group(1).count(",") + 1 == 4 and bat.group(1).count(",") + 1 == 21
    from boss_jl_amd import api
    so, sb = api.SIGNATURES["boss_gp_loglike_grad_mean"], api.SIGNATURES["boss_gp_loglike_grad_batch_mean"]
    assert so[0] is ctypes.c_int and sb[0] is ctypes.c_int and len(so[1]) == 4 and len(sb[1]) == 21
    dp = ctypes.POINTER(ctypes.c_double)
    # the gradient batch's arguments with (T, mean_jac, jac_stride) behind the parameters and the two outputs in front of the status
    old = api.SIGNATURES["boss_gp_loglike_grad_batch"][1]
    assert sb[1] == old[:13] + [ctypes.c_int, dp, ctypes.c_int] + old[13:15] + [dp, dp] + old[15:]
    assert so[1] == api.SIGNATURES["boss_gp_loglike_grad"][1] + [dp]

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return {"double": dp, "int": ctypes.POINTER(ctypes.c_int), "unsigned char": ctypes.POINTER(ctypes.c_ubyte),
                    "boss_gp_t": ctypes.c_void_p}[decl.replace("const", "").split("*")[0].strip()]
        return ctypes.c_int
    assert [ctype(p) for p in one.group(1).split(",")] == so[1] and [ctype(p) for p in bat.group(1).split(",")] == sb[1]
    import __graft_entry__ as entry
    entry.compile_library()
    lib = ctypes.CDLL(entry.LIB)
    assert hasattr(lib, "boss_gp_loglike_grad_mean") and hasattr(lib, "boss_gp_loglike_grad_batch_mean")


def test_wrapper_lays_out_shared_and_per_set_jacobians(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(0)
    d, N, S, T = 2, 5, 3, 4
    X, y = rng.uniform(0, 1, (d, N)), rng.standard_normal(N)
    lam, amp, sig = rng.uniform(0.3, 1.5, (d, S)), rng.uniform(0.5, 2, S), rng.uniform(0.05, 0.3, S)
    m_per, J_per, J_sh = rng.standard_normal((S, N)), rng.standard_normal((S, N, T)), rng.standard_normal((N, T))
    ll, st, gr, dm, dth = api.loglike_grad_batch_mean(np.ascontiguousarray(X), list(y), "matern32", np.ascontiguousarray(lam), amp, sig,
                                                      mean_X=np.asfortranarray(m_per), mean_jac=np.asfortranarray(J_per), device=1,
                                                      want_dmean=True)
    assert ll.tolist() == [-1.0, -2.0, -3.0] and st.dtype == np.int32 and not st.any()
    assert gr.shape == (d + 2, S) and all(gr[m, s] == 100.0 * s + m for s in range(S) for m in range(d + 2))
    assert dm.shape == (N, S) and all(dm[j, s] == 1000.0 * s + j for s in range(S) for j in range(N))       # column s = set s
    assert dth.shape == (T, S) and all(dth[t, s] == 10.0 * s + t for s in range(S) for t in range(T))
    a = fake.calls[-1]
    assert tuple(a[:4]) == (1, api.KERNELS["matern32"], d, N) and a[9] == S and a[7] == N and a[8] is None
    assert np.array_equal(a[4], X.reshape(-1, order="F")) and np.array_equal(a[6], m_per.reshape(-1))
    assert np.array_equal(a[10], lam.reshape(-1, order="F"))
    assert a[13] == T and a[15] == N * T
    for s in range(S):                                          # set after set, each N×T column-major: j runs fastest
        assert np.array_equal(a[14][s * N * T:(s + 1) * N * T], J_per[s].reshape(-1, order="F"))
    # one matrix shared by all sets; no mean values, no dmean
    ll, st, gr, dm, dth = api.loglike_grad_batch_mean(X, y, "matern32", lam, amp, sig, mean_jac=J_sh[:, ::-1], discrete=[True, False])
    a = fake.calls[-1]
    assert a[6] is None and a[7] == 0 and a[13] == T and a[15] == 0 and dm is None and dth.shape == (T, S)
    assert np.array_equal(a[14], J_sh[:, ::-1].reshape(-1, order="F"))
    # a shared mean vector, no Jacobian: no fold
    ll, st, gr, dm, dth = api.loglike_grad_batch_mean(X, y, "matern32", lam, amp, sig, mean_X=m_per[0], want_dmean=True)
    a = fake.calls[-1]
    assert a[7] == 0 and np.array_equal(a[6], m_per[0]) and a[13] == 0 and a[14] is None and a[15] == 0 and dth is None and dm.shape == (N, S)
    e = api.loglike_grad_batch_mean(X, y, "matern32", np.zeros((d, 0)), [], [], mean_jac=J_sh, want_dmean=True)
    assert e[0].shape == (0,) and e[2].shape == (d + 2, 0) and e[3].shape == (N, 0) and e[4].shape == (T, 0)


def test_wrapper_refuses_wrong_shapes(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(1)
    d, N, S, T = 2, 5, 3, 2
    X, y = rng.uniform(0, 1, (d, N)), rng.standard_normal(N)
    lam, amp, sig = rng.uniform(0.3, 1.5, (d, S)), rng.uniform(0.5, 2, S), rng.uniform(0.05, 0.3, S)
    J = rng.standard_normal((S, N, T))
    f = api.loglike_grad_batch_mean
    for bad in (lambda: f(X, y, "sqexp", lam, amp, sig, mean_jac=J[:2]),                    # S-1 sets
                lambda: f(X, y, "sqexp", lam, amp, sig, mean_jac=J.transpose(0, 2, 1)),      # S×T×N
                lambda: f(X, y, "sqexp", lam, amp, sig, mean_jac=J[0].T),                    # T×N
                lambda: f(X, y, "sqexp", lam, amp, sig, mean_jac=J[0, :, 0]),                # a vector
                lambda: f(X, y, "sqexp", lam, amp, sig, mean_jac=np.zeros((N, 0))),          # T = 0
                lambda: f(X, y, "sqexp", lam, amp, sig, mean_X=np.zeros((S - 1, N))),
                lambda: f(X, y, "sqexp", lam, amp, sig, mean_X=np.zeros(N + 1)),
                lambda: f(X, y, "sqexp", lam[:1], amp, sig),
                lambda: f(X, y, "sqexp", lam, amp[:2], sig),
                lambda: f(X, y[:-1], "sqexp", lam, amp, sig)):
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert not fake.calls                                        # none of the refused calls reached the library


def _affine(x, th):
    return np.array([th[0] + th[1] * x[0] - th[2] * x[1], 2.0 * th[0] - th[2]])


def _affine_jac(x, th):
    return np.array([[1.0, x[0], -x[1]], [2.0, 0.0, -1.0]])


def _nonlinear(x, th):
    return np.array([th[0] + th[1] * x[0] + np.cos(th[2] * x[1]), th[0] * th[1] * np.exp(-th[2] * x[0])])


def _nonlinear_jac(x, th):
    return np.array([[1.0, x[0], -x[1] * np.sin(th[2] * x[1])],
                     [th[1] * np.exp(-th[2] * x[0]), th[0] * np.exp(-th[2] * x[0]), -x[0] * th[0] * th[1] * np.exp(-th[2] * x[0])]])


def _model(B, P=2, parametric=_nonlinear, jac=None, theta_priors=None, d=2):
    return B.HipGaussianProcess(lengthscale_priors=[B.MvLogNormal([-0.5] * d, [0.4] * d)] * P, amplitude_priors=[B.LogNormal(0.0, 0.4)] * P,
                                noise_std_priors=[B.LogNormal(-2.0, 0.3)] * P, parametric=parametric, parametric_jac=jac,
                                theta_priors=[B.Normal(0.0, 2.0)] * 3 if theta_priors is None else theta_priors)


def test_central_difference_jacobian_matches_the_given_one():
    import boss_jl_amd as B
    rng = np.random.default_rng(2)
    X = rng.uniform(-1, 2, (2, 7))
    for fn, jac in ((_affine, _affine_jac), (_nonlinear, _nonlinear_jac)):
        for th in (np.array([0.3, -1.2, 0.7]), np.array([40.0, -1e-3, 2.5])):
            p = B.HipGPParams(np.ones((2, 2)), np.ones(2), np.ones(2), th)
            given, numeric = _model(B, parametric=fn, jac=jac), _model(B, parametric=fn)
            # central differences with steps h_t = 1e-6·max(1, |θ_t|): at most 16 roundings of 2⁻⁵³·max|m| over the smallest step's
            # 2h, and the truncation h²·|∂³m/∂θ³|/6 at the largest step with third derivatives below 60 (|x|³ ≤ 8, |θ0 θ1| ≤ 1)
            fmax = max(np.abs(fn(X[:, j], th)).max() for j in range(7))
            bound = 16 * 2.0 ** -53 * fmax / 2e-6 + (1e-6 * max(1.0, np.abs(th).max())) ** 2 * 10.0
            for i in range(2):
                Jg, Jn = given.mean_jacobians(X, p, i), numeric.mean_jacobians(X, p, i)
                assert Jg.shape == Jn.shape == (7, 3)
                assert np.array_equal(Jg, np.stack([jac(X[:, j], th)[i] for j in range(7)]))
                assert np.abs(Jg - Jn).max() <= bound, (np.abs(Jg - Jn).max(), bound)
    bad = _model(B, jac=lambda x, th: np.zeros((3, 2)))
    with pytest.raises(ValueError):
        bad.mean_jacobians(X, B.HipGPParams(np.ones((2, 2)), np.ones(2), np.ones(2), np.zeros(3)), 0)


def test_model_layer_sums_the_fold_over_the_outputs(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api
    rng = np.random.default_rng(3)
    d, N, P, S, T = 2, 6, 2, 4, 3
    data = B.ExperimentData(rng.uniform(0, 1, (d, N)), rng.standard_normal((P, N)))
    model = _model(B, P, _nonlinear, _nonlinear_jac)
    plist = [B.HipGPParams(rng.uniform(0.4, 0.8, (d, P)), rng.uniform(0.8, 1.4, P), rng.uniform(0.05, 0.1, P), rng.standard_normal(T))
             for _ in range(S)]
    avec = rng.standard_normal((P, S, N))                        # what the device would return as K⁻¹(y − m)
    seen = []

    def fake(X, y, kernel, lam, amp, sig, mean_X=None, mean_jac=None, discrete=None, device=0, want_dmean=False):
        i = len(seen)
        seen.append((X, y, kernel, lam, amp, sig, mean_X, mean_jac))
        st = np.zeros(S, dtype=np.int32)
        ll = np.arange(1.0, S + 1) * (i + 1)
        gr = np.arange((d + 2) * S, dtype=float).reshape(d + 2, S, order="F") + 1000.0 * (i + 1)
        dth = np.stack([mean_jac[s].T @ avec[i, s] for s in range(S)], axis=1)
        if i == 1:
            st[2], ll[2], gr[:, 2], dth[:, 2] = api.BOSS_E_NOT_PD, -np.inf, 0.0, 0.0
        return ll, st, gr, None, dth
    monkeypatch.setattr(api, "loglike_grad_batch_mean", fake)
    ll, grads = model.data_loglike_grad_batch(data, plist)
    assert len(seen) == P and ll.tolist() == [3.0, 6.0, -np.inf, 12.0] and len(grads) == S
    for i, (X, y, kernel, lam, amp, sig, mean_X, mean_jac) in enumerate(seen):
        assert np.array_equal(X, data.X) and np.array_equal(y, data.Y[i]) and kernel == "matern52"
        assert np.array_equal(lam, np.stack([p.lengthscales[:, i] for p in plist], axis=1))
        assert mean_X.shape == (S, N) and mean_jac.shape == (S, N, T)
        for s, p in enumerate(plist):                             # every set's own θ gives its mean row and its Jacobian
            assert np.array_equal(mean_X[s], [_nonlinear(data.X[:, j], p.theta)[i] for j in range(N)])
            assert np.array_equal(mean_jac[s], np.stack([_nonlinear_jac(data.X[:, j], p.theta)[i] for j in range(N)]))
    for s, (p, g) in enumerate(zip(plist, grads)):
        if s == 2:                                                # not PD in output 1: zeros in every group
            assert not g.lengthscales.any() and not g.amplitudes.any() and not g.noise_std.any() and not g.theta.any()
            continue
        want = sum(np.stack([_nonlinear_jac(data.X[:, j], p.theta)[i] for j in range(N)]).T @ avec[i, s] for i in range(P))
        assert np.allclose(g.theta, want, rtol=0, atol=1e-13) and g.theta.shape == (T,)
        for i in range(P):
            col = np.arange((d + 2) * s, (d + 2) * (s + 1), dtype=float) + 1000.0 * (i + 1)
            assert np.array_equal(g.lengthscales[:, i], col[:d]) and (g.amplitudes[i], g.noise_std[i]) == (col[d], col[d + 1])
    e_ll, e_g = model.data_loglike_grad_batch(data, [])
    assert e_ll.shape == (0,) and e_g == []
    # a model without a parametric mean: no Jacobian is passed, theta stays None
    plain = B.HipGaussianProcess(model.lengthscale_priors, model.amplitude_priors, model.noise_std_priors, mean=[0.5, -0.5])
    seen.clear()
    monkeypatch.setattr(api, "loglike_grad_batch_mean",
                        lambda X, y, k, lam, amp, sig, mean_X=None, mean_jac=None, discrete=None, device=0, want_dmean=False:
                        (seen.append((mean_X, mean_jac)), (np.zeros(S), np.zeros(S, dtype=np.int32), np.zeros((d + 2, S)), None, None))[1])
    _, g0 = plain.data_loglike_grad_batch(data, plist)
    assert all(g.theta is None for g in g0) and all(mj is None for _, mj in seen) and np.array_equal(seen[1][0], np.full(N, -0.5))


def test_normal_prior():
    import boss_jl_amd as B
    from boss_jl_amd.problem import Normal
    assert B.Normal is Normal
    pr = B.Normal(0.7, 1.9)
    for x in (-3.0, 0.0, 0.7, 5.5):
        h = 1e-5
        fd = (pr.logpdf(x + h) - pr.logpdf(x - h)) / (2 * h)
        assert abs(pr.grad_logpdf(x) - fd) <= 1e-8 * (1.0 + abs(fd))    # a quadratic: central differences are exact up to rounding
    assert abs(pr.logpdf(0.7) - (-np.log(1.9) - 0.5 * np.log(2 * np.pi))) < 1e-15
    draws = np.array([pr.rand(np.random.default_rng(5)) for _ in range(2)])
    assert draws[0] == draws[1] == 0.7 + 1.9 * np.random.default_rng(5).standard_normal()
    rng = np.random.default_rng(6)
    many = np.array([pr.rand(rng) for _ in range(4000)])
    assert abs(many.mean() - 0.7) < 0.15 and abs(many.std() - 1.9) < 0.15 and (many < 0).any()


def _concave_device(monkeypatch, api, calls=None):
    """A stand-in for the device call with a known maximum: -Σ log(λ, α, σ)² − ½‖y − m(θ)‖², so that the fold Jᵀa with
    a = y − m(θ) is its exact θ-gradient."""
    def fake(X, y, kernel, lam, amp, sig, mean_X=None, mean_jac=None, discrete=None, device=0, want_dmean=False):
        S = lam.shape[1]
        if calls is not None:
            calls.append(S)
        th = np.vstack([lam, amp[None], sig[None]])
        a = y[None, :] - mean_X
        ll = -(np.log(th) ** 2).sum(0) - 0.5 * (a ** 2).sum(1)
        dth = np.stack([mean_jac[s].T @ a[s] for s in range(S)], axis=1)
        return ll, np.zeros(S, dtype=np.int32), -2.0 * np.log(th) / th, None, dth
    monkeypatch.setattr(api, "loglike_grad_batch_mean", fake)


def _semipar_problem(B, theta_priors=None, seed=4, jac=_nonlinear_jac):
    rng = np.random.default_rng(seed)
    d, N, P = 2, 8, 2
    X = rng.uniform(0, 1, (d, N))
    truth = np.array([0.8, -0.6, 1.3])
    Y = np.stack([[_nonlinear(X[:, j], truth)[i] for j in range(N)] for i in range(P)])
    model = _model(B, P, _nonlinear, jac, theta_priors)
    prob = B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])), model,
                         B.ExperimentData(X, Y))
    return prob, truth


def test_fitter_moves_theta_and_keeps_dirac_entries(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api
    calls = []
    _concave_device(monkeypatch, api, calls)
    monkeypatch.setattr(api, "loglike_batch", lambda *a, **k: pytest.fail("the fixed-mean call on the Semiparametric route"))
    prob, truth = _semipar_problem(B)
    start = B.HipGradientMAP(multistart=4, iters=0, seed=2).estimate_parameters(prob, return_all=True)    # no longer raises
    n0 = len(calls)
    assert n0 == 2                                               # one call per output
    allp = B.HipGradientMAP(multistart=4, iters=25, seed=2).estimate_parameters(prob, return_all=True)
    assert len(allp) == 4 and all(a.loglike > s.loglike for a, s in zip(allp, start))
    assert all(not np.array_equal(a.params.theta, s.params.theta) for a, s in zip(allp, start))
    assert all(a.params.theta.shape == (3,) for a in allp)
    assert len(calls[n0:]) % 2 == 0 and all(c1 == c2 for c1, c2 in zip(calls[n0::2], calls[n0 + 1::2]))   # every round: one call per output
    # a Dirac entry stays; a positive-support entry moves in log-space and stays positive; a Normal entry may change sign
    priors = [B.Normal(0.0, 2.0), B.Dirac(-0.25), B.LogNormal(0.0, 0.5)]
    prob2, _ = _semipar_problem(B, priors)
    s2 = B.HipGradientMAP(multistart=3, iters=0, seed=3).estimate_parameters(prob2, return_all=True)
    a2 = B.HipGradientMAP(multistart=3, iters=25, seed=3).estimate_parameters(prob2, return_all=True)
    for a, s in zip(a2, s2):
        assert a.params.theta[1] == -0.25 == s.params.theta[1]
        assert a.params.theta[0] != s.params.theta[0] and a.params.theta[2] != s.params.theta[2] and a.params.theta[2] > 0
        assert a.loglike > s.loglike
    best = B.HipGradientMAP(multistart=3, iters=25, seed=3).estimate_parameters(prob2)
    assert best.loglike == max(a.loglike for a in a2)
    # the numeric Jacobian serves the same route
    prob3, _ = _semipar_problem(B, jac=None)
    a3 = B.HipGradientMAP(multistart=4, iters=25, seed=2).estimate_parameters(prob3, return_all=True)
    assert all(abs(a.loglike - b.loglike) <= 1e-6 * (1 + abs(a.loglike)) for a, b in zip(a3, allp))


def test_fitter_refuses_a_missing_theta_prior(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api
    monkeypatch.setattr(api, "loglike_grad_batch_mean", lambda *a, **k: pytest.fail("reached the device"))
    prob, _ = _semipar_problem(B, [B.Normal(0.0, 1.0), None, B.Normal(0.0, 1.0)])
    with pytest.raises(ValueError):
        B.HipGradientMAP(multistart=2, iters=1, seed=0, starts=[B.HipGPParams(np.ones((2, 2)), np.ones(2), np.ones(2), np.zeros(3))] * 2
                         ).estimate_parameters(prob)
    prob.model.theta_priors = None
    with pytest.raises(ValueError):
        B.HipGradientMAP(multistart=2, iters=1, seed=0, starts=[B.HipGPParams(np.ones((2, 2)), np.ones(2), np.ones(2), np.zeros(3))] * 2
                         ).estimate_parameters(prob)


def test_sample_opt_follows_and_plain_models_keep_their_route(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api
    _concave_device(monkeypatch, api)
    prob, _ = _semipar_problem(B)
    monkeypatch.setattr(B.HipGaussianProcess, "data_loglike_batch", lambda self, data, samples: np.array([-float(np.sum(s.theta ** 2)) for s in samples]))
    res = B.HipSampleOptMAP(samples=12, multistart=3, iters=5, seed=1).estimate_parameters(prob, return_all=True)
    assert len(res) == 3 and all(r.params.theta.shape == (3,) and np.isfinite(r.loglike) for r in res)
    # a model without a parametric mean still goes through loglike_batch(want_grad=True)
    seen = []

    def plain(X, y, kernel, lam, amp, sig, mean_X=None, discrete=None, device=0, want_grad=False):
        seen.append(want_grad)
        th = np.vstack([lam, amp[None], sig[None]])
        return -(np.log(th) ** 2).sum(0), np.zeros(lam.shape[1], dtype=np.int32), -2.0 * np.log(th) / th
    monkeypatch.setattr(api, "loglike_batch", plain)
    monkeypatch.setattr(api, "loglike_grad_batch_mean", lambda *a, **k: pytest.fail("the mean-gradient call on the plain route"))
    m = prob.model
    prob.model = B.HipGaussianProcess(m.lengthscale_priors, m.amplitude_priors, m.noise_std_priors)
    out = B.HipGradientMAP(multistart=2, iters=3, seed=1).estimate_parameters(prob)
    assert seen and all(seen) and out.params.theta is None


def test_winner_broadcast_carries_theta(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api
    from boss_jl_amd import distributed as dist_util
    _concave_device(monkeypatch, api)
    prob, _ = _semipar_problem(B)
    single = B.HipGradientMAP(multistart=4, iters=6, seed=2).estimate_parameters(prob, return_all=True)
    sent = {}
    # rank 1 of 2: it runs starts 2 and 3; the winner is made to be one of them, so this rank is the broadcast's source
    monkeypatch.setattr(dist_util, "rank_world", lambda group: (1, 2))
    monkeypatch.setattr(dist_util, "shared_seed", lambda seed, group: seed)
    monkeypatch.setattr(dist_util, "argmax_exchange", lambda v, i, group: (v, i))

    def bcast(flat, shape, owner, group):
        sent["flat"], sent["shape"], sent["owner"] = None if flat is None else flat.copy(), shape, owner
        return flat
    monkeypatch.setattr(dist_util, "broadcast_array", bcast)
    lo, hi = dist_util.shard_range(4, 1, 2)
    got = B.HipGradientMAP(multistart=4, iters=6, seed=2).estimate_parameters(prob)
    want = max(single[lo:hi], key=lambda r: r.loglike)
    d, P, T = 2, 2, 3
    assert sent["shape"] == (d * P + P + P + T,) and sent["owner"] == 1
    assert np.array_equal(sent["flat"][-T:], want.params.theta)                    # θ travels behind λ, α, σ
    assert np.array_equal(got.params.theta, want.params.theta) and np.array_equal(got.params.lengthscales, want.params.lengthscales)
    assert got.loglike == want.loglike
