"""Host-side checks of the batched likelihood gradients of the gradient-observation and the nonstationary model (no GPU): the
header, the signatures, the built library's exports, argument handling of the two Python wrappers against a fake library, the
model layer's summing and routing, the fitter over the batched model call, and the closures' evaluation points."""
import ctypes
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

    def boss_ggp_loglike_grad_batch(self, *a):
        assert len(a) == 15
        d, n, S = a[2], a[3], a[7]
        for s in range(S):
            a[12][s] = -1.0 - s
            a[14][s] = 0
            for m in range(d + 3):
                a[13][s * (d + 3) + m] = 100.0 * s + m            # column s of the (d+3)×S column-major gradient
        sizes = {4: d * n, 5: n, 6: d * n, 8: d * S, 9: S, 10: S, 11: S}
        self.calls.append(("ggp", tuple(_doubles(v, sizes[i]) if i in sizes else v for i, v in enumerate(a[:12]))))
        return 0

    def boss_ngp_loglike_grad_batch(self, *a):
        assert len(a) == 18
        d, N, S = a[1], a[2], a[6]
        for s in range(S):
            a[12][s] = -2.0 - s
            a[17][s] = 3 if s == 1 else 0
            for j in range(N):
                for k in range(d):
                    a[13][(s * N + j) * d + k] = 1000.0 * s + 10.0 * j + k   # set after set, each d×N column-major
                a[14][s * N + j] = 1.0 + s + 0.01 * j
                a[15][s * N + j] = 2.0 + s + 0.01 * j
                a[16][s * N + j] = 3.0 + s + 0.01 * j
        sizes = {3: d * N, 4: N, 7: d * N * S, 8: N * S, 9: N * S, 10: N * S if a[11] else N}
        rec = [_doubles(v, sizes[i]) if i in sizes else v for i, v in enumerate(a[:12])]
        rec[5] = None if a[5] is None else np.ctypeslib.as_array(a[5], shape=(d,)).copy()
        self.calls.append(("ngp", tuple(rec)))
        return 0


def test_header_signatures_and_library_agree():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bosship.h")).read(), flags=re.S)
    g = re.search(r"int\s+boss_ggp_loglike_grad_batch\s*\(([^;]*?)\);", hdr, re.S)
    n = re.search(r"int\s+boss_ngp_loglike_grad_batch\s*\(([^;]*?)\);", hdr, re.S)
    assert g and n
    assert g.group(1).count(",") + 1 == 15 and n.group(1).count(",") + 1 == 18
    from boss_jl_amd import api
    gs, ns = api.SIGNATURES["boss_ggp_loglike_grad_batch"], api.SIGNATURES["boss_ngp_loglike_grad_batch"]
    assert gs[0] is ctypes.c_int and ns[0] is ctypes.c_int and len(gs[1]) == 15 and len(ns[1]) == 18
    # the likelihood batches' arguments, the gradient outputs in front of the status
    lg, ln = api.SIGNATURES["boss_ggp_loglike_batch"][1], api.SIGNATURES["boss_ngp_loglike_batch"][1]
    dp = ctypes.POINTER(ctypes.c_double)
    assert gs[1] == lg[:13] + [dp] + lg[13:] and ns[1] == ln[:13] + [dp] * 4 + ln[13:]

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return {"double": dp, "int": ctypes.POINTER(ctypes.c_int), "unsigned char": ctypes.POINTER(ctypes.c_ubyte)}[
                decl.replace("const", "").split("*")[0].strip()]
        return ctypes.c_int
    assert [ctype(p) for p in g.group(1).split(",")] == gs[1] and [ctype(p) for p in n.group(1).split(",")] == ns[1]
    import __graft_entry__ as entry
    entry.compile_library()
    lib = ctypes.CDLL(entry.LIB)
    assert hasattr(lib, "boss_ggp_loglike_grad_batch") and hasattr(lib, "boss_ngp_loglike_grad_batch")


def test_ggp_grad_wrapper_checks_and_converts(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(0)
    d, n, S = 3, 5, 4
    X, y, dY = rng.uniform(0, 1, (d, n)), rng.standard_normal(n), rng.standard_normal((d, n))
    lam = rng.uniform(0.3, 1.5, (d, S))
    amp, sig, sgd = rng.uniform(0.5, 2, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
    ll, st, gr = api.ggp_loglike_grad_batch(np.ascontiguousarray(X), list(y), dY.astype(np.float32), "sqexp", np.ascontiguousarray(lam),
                                            amp.astype(np.float32), list(sig), sgd, device=2)
    assert ll.tolist() == [-1.0, -2.0, -3.0, -4.0] and st.dtype == np.int32 and not st.any()
    assert gr.shape == (d + 3, S) and all(gr[m, s] == 100.0 * s + m for s in range(S) for m in range(d + 3))
    name, a = fake.calls[-1]
    assert name == "ggp" and tuple(a[:4]) == (2, api.KERNELS["sqexp"], d, n) and a[7] == S
    assert np.array_equal(a[4], X.reshape(-1, order="F"))
    assert np.array_equal(a[6], dY.astype(np.float32).astype(np.float64).reshape(-1, order="F"))
    assert np.array_equal(a[8], lam.reshape(-1, order="F"))         # column s = set s
    assert np.array_equal(a[9], amp.astype(np.float32).astype(np.float64))
    assert np.array_equal(a[10], sig) and np.array_equal(a[11], sgd)
    for bad in (lambda: api.ggp_loglike_grad_batch(X, y, dY, "sqexp", lam[:2], amp, sig, sgd),
                lambda: api.ggp_loglike_grad_batch(X, y, dY, "sqexp", lam, amp[:3], sig, sgd),
                lambda: api.ggp_loglike_grad_batch(X, y, dY, "sqexp", lam, amp, sig, sgd[:1]),
                lambda: api.ggp_loglike_grad_batch(X, y[:4], dY, "sqexp", lam, amp, sig, sgd),
                lambda: api.ggp_loglike_grad_batch(X, y, dY[:2], "sqexp", lam, amp, sig, sgd),
                lambda: api.ggp_loglike_grad_batch(X, y, dY, "sqexp", lam[:, 0], amp, sig, sgd)):
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert len(fake.calls) == 1                                                    # none of the refused calls reached the library
    ll0, st0, gr0 = api.ggp_loglike_grad_batch(X, y, dY, "sqexp", np.zeros((d, 0)), [], [], [])
    assert ll0.shape == (0,) and st0.shape == (0,) and gr0.shape == (d + 3, 0)


def test_ngp_grad_wrapper_checks_and_converts(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(1)
    d, N, S = 2, 6, 3
    X, y = rng.uniform(0, 1, (d, N)), rng.standard_normal(N)
    lam, amp, noi = rng.uniform(0.3, 1, (d, N, S)), rng.uniform(0.5, 2, (N, S)), rng.uniform(0.05, 0.3, (N, S))
    ll, st, dl, da, dn, dm = api.ngp_loglike_grad_batch(X, y, np.ascontiguousarray(lam), amp.astype(np.float32), np.ascontiguousarray(noi))
    assert ll.tolist() == [-2.0, -3.0, -4.0] and st.tolist() == [0, 3, 0]
    assert dl.shape == (d, N, S) and da.shape == dn.shape == dm.shape == (N, S)
    for s in range(S):
        for j in range(N):
            assert [dl[k, j, s] for k in range(d)] == [1000.0 * s + 10.0 * j + k for k in range(d)]
            assert (da[j, s], dn[j, s], dm[j, s]) == (1.0 + s + 0.01 * j, 2.0 + s + 0.01 * j, 3.0 + s + 0.01 * j)
    name, a = fake.calls[-1]
    assert name == "ngp" and tuple(a[:3]) == (0, d, N) and a[5] is None and a[6] == S and a[10] is None and a[11] == 0
    for s in range(S):                                                             # set after set, each d×N column-major
        assert np.array_equal(a[7][s * d * N:(s + 1) * d * N], lam[:, :, s].reshape(-1, order="F"))
    assert np.array_equal(a[8], amp.astype(np.float32).astype(np.float64).reshape(-1, order="F"))
    assert np.array_equal(a[9], noi.reshape(-1, order="F"))
    m_shared, m_per = rng.standard_normal(N), rng.standard_normal((S, N))
    api.ngp_loglike_grad_batch(X, y, lam, amp, noi, mean_X=m_shared, discrete=[True, False], device=1)
    a = fake.calls[-1][1]
    assert a[0] == 1 and a[11] == 0 and np.array_equal(a[10], m_shared) and a[5].tolist() == [1, 0]
    api.ngp_loglike_grad_batch(X, y, lam, amp, noi, mean_X=np.asfortranarray(m_per))
    a = fake.calls[-1][1]
    assert a[11] == N and np.array_equal(a[10], m_per.reshape(-1))
    n_ok = len(fake.calls)
    X17 = rng.uniform(0, 1, (17, N))
    for bad in (lambda: api.ngp_loglike_grad_batch(X, y, lam[:, :, 0], amp, noi),
                lambda: api.ngp_loglike_grad_batch(X, y, lam.transpose(2, 0, 1), amp, noi),
                lambda: api.ngp_loglike_grad_batch(X, y, lam, amp.T, noi),
                lambda: api.ngp_loglike_grad_batch(X, y, lam, amp, noi[:, :2]),
                lambda: api.ngp_loglike_grad_batch(X, y[:-1], lam, amp, noi),
                lambda: api.ngp_loglike_grad_batch(X, y, lam, amp, noi, mean_X=m_per[:2]),
                lambda: api.ngp_loglike_grad_batch(X, y, lam, amp, noi, discrete=[True]),
                lambda: api.ngp_loglike_grad_batch(X17, y, np.ones((17, N, S)), amp, noi)):           # x_dim above 16
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert len(fake.calls) == n_ok
    e = api.ngp_loglike_grad_batch(X, y, np.zeros((d, N, 0)), np.zeros((N, 0)), np.zeros((N, 0)))
    assert e[0].shape == (0,) and e[2].shape == (d, N, 0) and e[3].shape == (N, 0)


def _gradient_problem(B, P=2, d=2, n=6, seed=3):
    rng = np.random.default_rng(seed)
    data = B.GradientData(rng.uniform(0, 1, (d, n)), rng.standard_normal((P, n)), rng.standard_normal((P, d, n)))
    return rng, data


def test_gradient_model_sums_outputs_and_zeroes_failed_sets(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api, gradient_gp
    d, n, P, S = 2, 6, 2, 5
    rng, data = _gradient_problem(B, P, d, n)
    prm = [B.HipGradientGPParams(rng.uniform(0.4, 0.8, (d, P)), rng.uniform(0.8, 1.4, P), rng.uniform(0.02, 0.06, P),
                                 rng.uniform(0.05, 0.2, P)) for _ in range(S)]
    model = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P, kernel="matern32", device=0)
    seen = []

    def fake(X, y, dY, kernel, lam, amp, sig, sgd, device=0):
        seen.append((X, y, dY, kernel, lam, amp, sig, sgd, device))
        i = len(seen)
        st = np.zeros(S, dtype=np.int32)
        gr = np.arange((d + 3) * S, dtype=float).reshape(d + 3, S, order="F") + 1000.0 * i
        ll = np.arange(1.0, S + 1) * i
        if i == 2:
            st[3], ll[3], gr[:, 3] = api.BOSS_E_NOT_PD, -np.inf, 0.0
        return ll, st, gr
    monkeypatch.setattr(api, "ggp_loglike_grad_batch", fake)
    monkeypatch.setattr(api, "GradGP", lambda *a, **k: pytest.fail("a handle was created on the batched route"))
    monkeypatch.setattr(gradient_gp, "batched_grad_call_pays", lambda rows, n_sets: True)
    ll, grads = model.data_loglike_grad_batch(data, prm)
    assert len(seen) == P and ll.tolist() == [3.0, 6.0, 9.0, -np.inf, 15.0] and len(grads) == S
    for i, (X, y, dY, kernel, lam, amp, sig, sgd, device) in enumerate(seen):
        assert np.array_equal(X, data.X) and np.array_equal(y, data.Y[i]) and np.array_equal(dY, data.dY[i]) and kernel == "matern32"
        assert np.array_equal(lam, np.stack([p.lengthscales[:, i] for p in prm], axis=1))
        assert amp.tolist() == [p.amplitudes[i] for p in prm] and sgd.tolist() == [p.grad_noise_std[i] for p in prm]
    for s, g in enumerate(grads):
        assert g.lengthscales.shape == (d, P) and g.amplitudes.shape == (P,)
        if s == 3:                                                # not PD in output 1: zeros in BOTH outputs
            assert not g.lengthscales.any() and not g.amplitudes.any() and not g.noise_std.any() and not g.grad_noise_std.any()
            continue
        for i in range(P):
            col = np.arange((d + 3) * s, (d + 3) * (s + 1), dtype=float) + 1000.0 * (i + 1)
            assert np.array_equal(g.lengthscales[:, i], col[:d])
            assert (g.amplitudes[i], g.noise_std[i], g.grad_noise_std[i]) == (col[d], col[d + 1], col[d + 2])
    e_ll, e_g = model.data_loglike_grad_batch(data, [])
    assert e_ll.shape == (0,) and e_g == []


def test_gradient_model_keeps_the_loop_where_the_batch_does_not_pay(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api, gradient_gp
    d, n, P, S = 2, 6, 2, 3
    rng, data = _gradient_problem(B, P, d, n)
    prm = [B.HipGradientGPParams(np.full((d, P), 0.5 + s), np.ones(P), np.full(P, 0.1), np.full(P, 0.1)) for s in range(S)]
    made = []

    class FakeHandle:
        def __init__(self, X, y, dY, kernel="matern52", device=0):
            self.closed = False
            made.append(self)

        def update(self, lam, amp, sig, sgd):
            self.lam0 = float(lam[0])
            if self.lam0 == 1.5 and self is made[1]:
                raise api.PosDefException(api.BOSS_E_NOT_PD, "not PD")
            return self.lam0

        def loglike_grad(self):
            return self.lam0, np.full(d + 3, self.lam0)

        def close(self):
            self.closed = True
    monkeypatch.setattr(api, "GradGP", FakeHandle)
    monkeypatch.setattr(api, "ggp_loglike_grad_batch", lambda *a, **k: pytest.fail("batched call on the loop's route"))
    pays = gradient_gp.batched_grad_call_pays                      # the shipped predicate, checked at the end
    monkeypatch.setattr(gradient_gp, "batched_grad_call_pays", lambda rows, n_sets: False)
    model = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P)
    ll, grads = model.data_loglike_grad_batch(data, prm)
    assert len(made) == P and all(h.closed for h in made)          # one resident handle per output, closed afterwards
    assert ll.tolist() == [1.0, -np.inf, 5.0] and not grads[1].lengthscales.any() and grads[2].amplitudes.tolist() == [2.5, 2.5]
    # unmeasured shapes keep the loop; a single set is never a batch
    assert not pays(60, 1) and not pays(10 ** 6, 64)
    assert pays(60, 8) and pays(4095, 64)                         # the measured region
    assert not pays(60, 7) and not pays(4096, 64)


def test_gradient_map_makes_one_batched_call_per_output_per_round(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api, gradient_gp
    d, n, P = 2, 5, 2
    rng, data = _gradient_problem(B, P, d, n, seed=4)
    model = B.HipGradientGaussianProcess(lengthscale_priors=[B.MvLogNormal([-0.5] * d, [0.4] * d)] * P,
                                         amplitude_priors=[B.LogNormal(0.0, 0.4)] * P, noise_std_priors=[B.LogNormal(-3.0, 0.3)] * P,
                                         grad_noise_std_priors=[B.LogNormal(-2.0, 0.3)] * P)
    calls = []

    def fake(X, y, dY, kernel, lam, amp, sig, sgd, device=0):
        S = lam.shape[1]
        calls.append(S)
        # a concave objective in log-parameters with its exact gradient: -Σ log(θ)²
        th = np.vstack([lam, amp[None], sig[None], sgd[None]])
        return -(np.log(th) ** 2).sum(0), np.zeros(S, dtype=np.int32), -2.0 * np.log(th) / th
    monkeypatch.setattr(api, "ggp_loglike_grad_batch", fake)
    monkeypatch.setattr(api, "GradGP", lambda *a, **k: pytest.fail("a handle was created on the batched route"))
    monkeypatch.setattr(gradient_gp, "batched_grad_call_pays", lambda rows, n_sets: True)
    monkeypatch.setattr(B.HipGradientGaussianProcess, "params_loglike", lambda self: (lambda p: 0.0))
    for pr in (B.MvLogNormal, B.LogNormal):
        monkeypatch.setattr(pr, "grad_logpdf", lambda self, x: np.zeros_like(np.asarray(x, float)))
    rounds = []
    real = B.HipGradientMAP._objective_gradient_model
    monkeypatch.setattr(B.HipGradientMAP, "_objective_gradient_model",
                        lambda self, *a: (rounds.append(len(a[-1])), real(self, *a))[1])
    prob = B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])), model, data)
    allp = B.HipGradientMAP(multistart=4, iters=3, seed=2).estimate_parameters(prob, return_all=True)
    assert len(allp) == 4 and rounds[0] == 4 and len(rounds) >= 2
    assert calls == [s for s in rounds for _ in range(P)]         # every round: one call per output, all of the round's starts in it
    start = B.HipGradientMAP(multistart=4, iters=0, seed=2).estimate_parameters(prob, return_all=True)
    assert all(a.loglike > s.loglike for a, s in zip(allp, start))  # the ascent climbed from every start


def test_nonstationary_grad_batch_evaluates_closures_like_latent_at_data(monkeypatch):
    """λ(·), α(·) at the ROUNDED points of the discrete dimensions, σ(·) and the prior mean at the points as given — what
    HipNonstationaryGP._latent_at_data yields — for every model of the batch, one call per output."""
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
        i = len(seen)
        st = np.zeros(S, dtype=np.int32)
        st[2] = api.BOSS_E_NOT_PD if i == 2 else 0
        ll = np.array([1.0, 2.0, 3.0]) * i
        out = [np.full((d, N, S), 10.0 * i), np.full((N, S), 20.0 * i), np.full((N, S), 30.0 * i), np.full((N, S), 40.0 * i)]
        for s in range(S):
            for a in out:
                a[..., s] += s
        return (ll, st, *out)
    monkeypatch.setattr(api, "ngp_loglike_grad_batch", fake)
    tot, grads = nonstationary.data_loglike_grad_batch(models, data)
    assert len(seen) == P and tot.tolist() == [3.0, 6.0, -np.inf]
    Xr = X.copy()
    Xr[1] = np.rint(Xr[1])
    assert not np.array_equal(Xr, X)
    for i, (Xa, y, lam, amp, noi, mean_X, discrete, device) in enumerate(seen):
        assert np.array_equal(Xa, X) and np.array_equal(y, data.Y[i]) and list(discrete) == disc and device == 0
        for s, m in enumerate(models):
            l1, a1, n1, m1, _ = m._latent_at_data(X, i)
            assert np.array_equal(lam[:, :, s], l1) and np.array_equal(amp[:, s], a1) and np.array_equal(noi[:, s], n1)
            c = (1.0, 2.0, 3.0)[s]
            assert np.array_equal(lam[:, :, s], c * (0.3 + 0.1 * Xr ** 2))           # rounded points for λ and α
            assert np.array_equal(amp[:, s], 1.0 + c * Xr[1]) and np.array_equal(noi[:, s], 0.1 * c + 0.01 * X[1])   # raw for σ
        if i == 0:                                                                 # the mean at the raw points
            assert mean_X.shape == (S, N) and np.array_equal(mean_X[0], X[1]) and not mean_X[1].any() and np.array_equal(mean_X[2], 3.0 * X[1])
        else:
            assert mean_X is None
    for s in range(2):
        for i in range(P):
            dl, da, dn, dm = grads[s][i]
            assert dl.shape == (d, N) and (dl == 10.0 * (i + 1) + s).all() and (da == 20.0 * (i + 1) + s).all()
            assert (dn == 30.0 * (i + 1) + s).all() and (dm == 40.0 * (i + 1) + s).all()
    assert all(not a.any() for i in range(P) for a in grads[2][i])                   # not PD in one output: zero cotangents in both
    e_tot, e_g = nonstationary.data_loglike_grad_batch([], data)
    assert e_tot.shape == (0,) and e_g == []
    with pytest.raises(ValueError):
        nonstationary.data_loglike_grad_batch([models[0], B.HipNonstationaryGP(models[0].f_lam, models[0].f_amp, models[0].f_noise)], data)
    assert B.nonstationary_data_loglike_grad_batch is nonstationary.data_loglike_grad_batch
