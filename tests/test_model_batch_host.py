"""Host-side checks of the batched likelihoods of the gradient-observation and the nonstationary model (no GPU): argument
handling of the two Python wrappers, the header, the closures' evaluation points, and the fitter over the batched model call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _doubles(ptr, n):
    return None if ptr is None else np.ctypeslib.as_array(ptr, shape=(n,)).copy()


class _FakeLib:
    """Stands in for libbosship.so: copies what the wrappers pass (the arrays live only during the call) and fills the outputs."""

    def __init__(self):
        self.calls = []

    def boss_ggp_loglike_batch(self, *a):
        d, n, S = a[2], a[3], a[7]
        for s in range(S):
            a[12][s] = -1.0 - s
            a[13][s] = 0
        sizes = {4: d * n, 5: n, 6: d * n, 8: d * S, 9: S, 10: S, 11: S}
        self.calls.append(("ggp", tuple(_doubles(v, sizes[i]) if i in sizes else v for i, v in enumerate(a[:12]))))
        return 0

    def boss_ngp_loglike_batch(self, *a):
        d, N, S = a[1], a[2], a[6]
        for s in range(S):
            a[12][s] = -2.0 - s
            a[13][s] = 3 if s == 1 else 0
        sizes = {3: d * N, 4: N, 7: d * N * S, 8: N * S, 9: N * S, 10: N * S if a[11] else N}
        rec = [_doubles(v, sizes[i]) if i in sizes else v for i, v in enumerate(a[:12])]
        rec[5] = None if a[5] is None else np.ctypeslib.as_array(a[5], shape=(d,)).copy()
        self.calls.append(("ngp", tuple(rec)))
        return 0


def test_header_declares_both_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bosship.h")).read(), flags=re.S)
    g = re.search(r"int\s+boss_ggp_loglike_batch\s*\(([^;]*?)\);", hdr, re.S)
    n = re.search(r"int\s+boss_ngp_loglike_batch\s*\(([^;]*?)\);", hdr, re.S)
    assert g and n
    assert g.group(1).count(",") + 1 == 14 and n.group(1).count(",") + 1 == 14
    from boss_jl_amd import api
    assert len(api.SIGNATURES["boss_ggp_loglike_batch"][1]) == 14 and len(api.SIGNATURES["boss_ngp_loglike_batch"][1]) == 14


def test_ggp_wrapper_checks_and_converts(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(0)
    d, n, S = 3, 5, 4
    X, y, dY = rng.uniform(0, 1, (d, n)), rng.standard_normal(n), rng.standard_normal((d, n))
    lam = rng.uniform(0.3, 1.5, (d, S))
    amp, sig, sgd = rng.uniform(0.5, 2, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
    # C-ordered, float32 and list inputs all reach the ABI as column-major float64
    ll, st = api.ggp_loglike_batch(np.ascontiguousarray(X), list(y), dY.astype(np.float32), "sqexp", np.ascontiguousarray(lam),
                                   amp.astype(np.float32), list(sig), sgd, device=2)
    assert ll.tolist() == [-1.0, -2.0, -3.0, -4.0] and st.dtype == np.int32 and not st.any()
    name, a = fake.calls[-1]
    assert name == "ggp" and tuple(a[:4]) == (2, api.KERNELS["sqexp"], d, n) and a[7] == S
    assert np.array_equal(a[4], X.reshape(-1, order="F"))
    assert np.array_equal(a[6], dY.astype(np.float32).astype(np.float64).reshape(-1, order="F"))
    assert np.array_equal(a[8], lam.reshape(-1, order="F"))         # column s = set s
    assert np.array_equal(a[9], amp.astype(np.float32).astype(np.float64))
    assert np.array_equal(a[10], sig) and np.array_equal(a[11], sgd)
    for bad in (lambda: api.ggp_loglike_batch(X, y, dY, "sqexp", lam[:2], amp, sig, sgd),             # lengthscales not d×S
                lambda: api.ggp_loglike_batch(X, y, dY, "sqexp", lam, amp[:3], sig, sgd),             # one amplitude short
                lambda: api.ggp_loglike_batch(X, y, dY, "sqexp", lam, amp, sig, sgd[:1]),
                lambda: api.ggp_loglike_batch(X, y[:4], dY, "sqexp", lam, amp, sig, sgd),
                lambda: api.ggp_loglike_batch(X, y, dY[:2], "sqexp", lam, amp, sig, sgd),
                lambda: api.ggp_loglike_batch(X, y, dY, "sqexp", lam[:, 0], amp, sig, sgd)):          # a vector is not d×S
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert len(fake.calls) == 1                                                    # none of the refused calls reached the library
    ll0, st0 = api.ggp_loglike_batch(X, y, dY, "sqexp", np.zeros((d, 0)), [], [], [])
    assert ll0.shape == (0,) and st0.shape == (0,)


def test_ngp_wrapper_checks_and_converts(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(1)
    d, N, S = 2, 6, 3
    X, y = rng.uniform(0, 1, (d, N)), rng.standard_normal(N)
    lam, amp, noi = rng.uniform(0.3, 1, (d, N, S)), rng.uniform(0.5, 2, (N, S)), rng.uniform(0.05, 0.3, (N, S))
    ll, st = api.ngp_loglike_batch(X, y, np.ascontiguousarray(lam), amp.astype(np.float32), np.ascontiguousarray(noi))
    assert ll.tolist() == [-2.0, -3.0, -4.0] and st.tolist() == [0, 3, 0]
    name, a = fake.calls[-1]
    assert name == "ngp" and tuple(a[:3]) == (0, d, N) and a[5] is None and a[6] == S and a[10] is None and a[11] == 0
    got = a[7]
    for s in range(S):                                                             # set after set, each d×N column-major
        assert np.array_equal(got[s * d * N:(s + 1) * d * N], lam[:, :, s].reshape(-1, order="F"))
    assert np.array_equal(a[8], amp.astype(np.float32).astype(np.float64).reshape(-1, order="F"))
    assert np.array_equal(a[9], noi.reshape(-1, order="F"))
    # prior means: shared (N, stride 0) or per set (S×N rows, stride N); discrete flags as bytes
    m_shared, m_per = rng.standard_normal(N), rng.standard_normal((S, N))
    api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=m_shared, discrete=[True, False], device=1)
    a = fake.calls[-1][1]
    assert a[0] == 1 and a[11] == 0 and np.array_equal(a[10], m_shared)
    assert a[5].tolist() == [1, 0]
    api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=np.asfortranarray(m_per))
    a = fake.calls[-1][1]
    assert a[11] == N and np.array_equal(a[10], m_per.reshape(-1))
    n_ok = len(fake.calls)
    for bad in (lambda: api.ngp_loglike_batch(X, y, lam[:, :, 0], amp, noi),                          # d×N is not d×N×S
                lambda: api.ngp_loglike_batch(X, y, lam.transpose(2, 0, 1), amp, noi),                # S×d×N
                lambda: api.ngp_loglike_batch(X, y, lam, amp.T, noi),                                 # S×N
                lambda: api.ngp_loglike_batch(X, y, lam, amp, noi[:, :2]),
                lambda: api.ngp_loglike_batch(X, y, lam, amp[:, 0], noi),
                lambda: api.ngp_loglike_batch(X, y[:-1], lam, amp, noi),
                lambda: api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=m_per[:2]),
                lambda: api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=m_shared[:-1]),
                lambda: api.ngp_loglike_batch(X, y, lam, amp, noi, discrete=[True])):
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert len(fake.calls) == n_ok


def test_nonstationary_batch_evaluates_closures_like_latent_at_data(monkeypatch):
    """λ(·), α(·) at the ROUNDED points of the discrete dimensions, σ(·) and the prior mean at the points as given — what
    HipNonstationaryGP._latent_at_data hands to the single-handle path — for every model of the batch, one call per output."""
    import boss_jl_amd as B
    from boss_jl_amd import api, nonstationary
    rng = np.random.default_rng(2)
    d, N, P, S = 2, 7, 2, 3
    X = rng.uniform(0, 4, (d, N))
    data = B.ExperimentData(X, rng.standard_normal((P, N)))
    disc = [False, True]

    def model(c):
        return B.HipNonstationaryGP(f_lam=[lambda x, c=c: c * (0.3 + 0.1 * np.asarray(x) ** 2)] * P, f_amp=[lambda x, c=c: 1.0 + c * x[1]] * P,
                                    f_noise=[lambda x, c=c: 0.1 * c + 0.01 * x[1]] * P,
                                    mean=None if c == 2.0 else [lambda x, c=c: c * x[1], None], discrete=disc)
    models = [model(c) for c in (1.0, 2.0, 3.0)]
    seen = []

    def fake(Xa, y, lam, amp, noi, mean_X=None, discrete=None, device=0):
        seen.append((Xa, y, lam.copy(), amp.copy(), noi.copy(), mean_X, discrete, device))
        st = np.zeros(S, dtype=np.int32)
        st[2] = api.BOSS_E_NOT_PD if len(seen) == 2 else 0
        return np.array([1.0, 2.0, 3.0]) * len(seen), st
    monkeypatch.setattr(api, "ngp_loglike_batch", fake)
    out = nonstationary.data_loglike_batch(models, data)
    assert len(seen) == P and out.tolist() == [3.0, 6.0, -np.inf]                    # summed over outputs, -inf where one is not PD
    Xr = X.copy()
    Xr[1] = np.rint(Xr[1])
    assert not np.array_equal(Xr, X)
    for i, (Xa, y, lam, amp, noi, mean_X, discrete, device) in enumerate(seen):
        assert np.array_equal(Xa, X) and np.array_equal(y, data.Y[i]) and list(discrete) == disc and device == 0
        assert lam.shape == (d, N, S) and amp.shape == (N, S) and noi.shape == (N, S)
        for s, m in enumerate(models):
            l1, a1, n1, m1, _ = m._latent_at_data(X, i)
            assert np.array_equal(lam[:, :, s], l1) and np.array_equal(amp[:, s], a1) and np.array_equal(noi[:, s], n1)
            c = (1.0, 2.0, 3.0)[s]
            assert np.array_equal(amp[:, s], 1.0 + c * Xr[1]) and np.array_equal(noi[:, s], 0.1 * c + 0.01 * X[1])
        if i == 0:                                                                 # models 0 and 2 carry a mean for output 0, model 1 none
            assert mean_X.shape == (S, N) and np.array_equal(mean_X[0], X[1]) and not mean_X[1].any() and np.array_equal(mean_X[2], 3.0 * X[1])
        else:
            assert mean_X is None
    assert nonstationary.data_loglike_batch([], data).shape == (0,)
    with pytest.raises(ValueError):
        nonstationary.data_loglike_batch([models[0], B.HipNonstationaryGP(models[0].f_lam, models[0].f_amp, models[0].f_noise)], data)
    with pytest.raises(ValueError):
        nonstationary.data_loglike_batch([models[0], B.HipNonstationaryGP(models[0].f_lam, models[0].f_amp, models[0].f_noise,
                                                                          discrete=disc, device=1)], data)
    assert B.nonstationary_data_loglike_batch is nonstationary.data_loglike_batch


def test_gradient_model_routes_batches_and_sums_outputs(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api, gradient_gp
    rng = np.random.default_rng(3)
    d, n, P, S = 2, 6, 2, 5
    data = B.GradientData(rng.uniform(0, 1, (d, n)), rng.standard_normal((P, n)), rng.standard_normal((P, d, n)))
    prm = [B.HipGradientGPParams(rng.uniform(0.4, 0.8, (d, P)), rng.uniform(0.8, 1.4, P), rng.uniform(0.02, 0.06, P),
                                 rng.uniform(0.05, 0.2, P)) for _ in range(S)]
    model = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P, kernel="matern32", device=0)
    seen = []

    def fake(X, y, dY, kernel, lam, amp, sig, sgd, device=0):
        seen.append((X, y, dY, kernel, lam, amp, sig, sgd, device))
        st = np.zeros(S, dtype=np.int32)
        if len(seen) == 2:
            st[3] = api.BOSS_E_NOT_PD
        return np.arange(1.0, S + 1) * len(seen), st
    monkeypatch.setattr(api, "ggp_loglike_batch", fake)
    assert gradient_gp.batched_call_pays(n * (1 + d), S)
    out = model.data_loglike_batch(data, prm)
    assert len(seen) == P and out.tolist() == [3.0, 6.0, 9.0, -np.inf, 15.0]
    for i, (X, y, dY, kernel, lam, amp, sig, sgd, device) in enumerate(seen):
        assert np.array_equal(X, data.X) and np.array_equal(y, data.Y[i]) and np.array_equal(dY, data.dY[i]) and kernel == "matern32"
        assert np.array_equal(lam, np.stack([p.lengthscales[:, i] for p in prm], axis=1))
        assert amp.tolist() == [p.amplitudes[i] for p in prm] and sig.tolist() == [p.noise_std[i] for p in prm]
        assert sgd.tolist() == [p.grad_noise_std[i] for p in prm]
    assert model.data_loglike_batch(data, []).shape == (0,)
    # the switch-over is one predicate: a single set is never a batch, many sets of a fitter-sized system always are
    assert not gradient_gp.batched_call_pays(60, 1) and gradient_gp.batched_call_pays(60, 64) and gradient_gp.batched_call_pays(1017, 512)


def test_batched_map_over_gradient_model_keeps_the_first_best_sample(monkeypatch):
    """sampling_optim (sampling.jl:59-71): strict `>` keeps the FIRST best sample — HipBatchedMAP over a HipGradientGaussianProcess
    whose data_loglike_batch is replaced by a fake with a tie."""
    import boss_jl_amd as B
    d, n, P = 2, 5, 1
    rng = np.random.default_rng(4)
    data = B.GradientData(rng.uniform(0, 1, (d, n)), rng.standard_normal((P, n)), rng.standard_normal((P, d, n)))
    model = B.HipGradientGaussianProcess(lengthscale_priors=[B.MvDirac([0.5] * d)] * P, amplitude_priors=[B.LogNormal(0.0, 0.5)] * P,
                                         noise_std_priors=[B.Dirac(0.05)] * P, grad_noise_std_priors=[B.Dirac(0.1)] * P)
    calls = []

    def fake(self, data_, samples):
        calls.append(len(samples))
        return np.array([-5.0, 1.0, -2.0, 1.0, 0.5, 1.0, -9.0])[:len(samples)]    # ties at draws 1, 3, 5
    monkeypatch.setattr(B.HipGradientGaussianProcess, "data_loglike_batch", fake)
    monkeypatch.setattr(B.HipGradientGaussianProcess, "params_loglike", lambda self: (lambda p: 0.0))   # the log-posterior is the fake's value
    prob = B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0])), model, data)
    fit = B.HipBatchedMAP(samples=7, seed=3)
    allp = fit.estimate_parameters(prob, return_all=True)
    best = fit.estimate_parameters(prob)
    assert calls == [7, 7] and len(allp) == 7
    assert best.loglike == pytest.approx(1.0, abs=1e-12)
    assert np.array_equal(best.params.amplitudes, allp[1].params.amplitudes)         # the first of the tied draws
    assert not np.array_equal(allp[1].params.amplitudes, allp[3].params.amplitudes)
