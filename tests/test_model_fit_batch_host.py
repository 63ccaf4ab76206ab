"""Host-side checks of the fitted sets of the gradient-observation and the nonstationary model and of the set-wide prediction
(no GPU): the header and the ctypes signatures, argument handling of the three Python wrappers, and the routing of
`model_posterior(list)` / `nonstationary_model_posterior_batch` / `nonstationary_acq_ei_batch` through the batch entry points."""
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

    def boss_ggp_fit_batch(self, *a):
        d, n, S = a[2], a[3], a[7]
        for s in range(S):
            a[12][s] = 1000 + s
            a[13][s] = -1.0 - s
            a[14][s] = 3 if s == 1 else 0
        sizes = {4: d * n, 5: n, 6: d * n, 8: d * S, 9: S, 10: S, 11: S}
        self.calls.append(("ggp_fit", tuple(_doubles(v, sizes[i]) if i in sizes else v for i, v in enumerate(a[:12]))))
        return 0

    def boss_ngp_fit_batch(self, *a):
        d, N, S = a[1], a[2], a[6]
        for s in range(S):
            a[12][s] = 2000 + s
            a[13][s] = -2.0 - s
            a[14][s] = 0
        sizes = {3: d * N, 4: N, 7: d * N * S, 8: N * S, 9: N * S, 10: N * S if a[11] else N}
        rec = [_doubles(v, sizes[i]) if i in sizes else v for i, v in enumerate(a[:12])]
        rec[5] = None if a[5] is None else np.ctypeslib.as_array(a[5], shape=(d,)).copy()
        self.calls.append(("ngp_fit", tuple(rec)))
        return 0

    def boss_ngp_predict_set(self, n, gps, M, Xs, lam, amp, mean, mu, var, bad):
        d = self.d
        self.calls.append(("ngp_set", (n, [gps[i] for i in range(n)], M, _doubles(Xs, d * M), _doubles(lam, d * M * n), _doubles(amp, M * n),
                                       _doubles(mean, M * n))))
        for k in range(n * M):
            mu[k] = float(k)
            var[k] = 0.5 + k
        return 0

    def boss_gp_free(self, h):
        self.calls.append(("free", h.value if hasattr(h, "value") else h))


def _nargs(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bosship.h")).read(), flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^;]*?)\);", hdr, re.S)
    assert m, name + " is not declared in include/bosship.h"
    return m.group(1).count(",") + 1


def test_header_declares_the_three_symbols():
    from boss_jl_amd import api
    for name, n in (("boss_ggp_fit_batch", 15), ("boss_ngp_fit_batch", 15), ("boss_ngp_predict_set", 10)):
        assert _nargs(name) == n, name
        assert len(api.SIGNATURES[name][1]) == n, name
    # the fit batches take the arguments of the likelihood batches, with the handle array in front of the outputs
    assert api.SIGNATURES["boss_ggp_fit_batch"][1][:12] == api.SIGNATURES["boss_ggp_loglike_batch"][1][:12]
    assert api.SIGNATURES["boss_ngp_fit_batch"][1][:12] == api.SIGNATURES["boss_ngp_loglike_batch"][1][:12]
    jl = open(os.path.join(ROOT, "boss.jl_amd", "julia", "BOSSHip.jl")).read()
    for name in ("boss_ggp_fit_batch", "boss_ngp_fit_batch", "boss_ngp_predict_set"):
        assert "(:%s, lib)" % name in jl, name


def test_ggp_fit_batch_wrapper_checks_and_converts(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(0)
    d, n, S = 3, 5, 4
    X, y, dY = rng.uniform(0, 1, (d, n)), rng.standard_normal(n), rng.standard_normal((d, n))
    lam = rng.uniform(0.3, 1.5, (d, S))
    amp, sig, sgd = rng.uniform(0.5, 2, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
    gps, ll, st = api.ggp_fit_batch(np.ascontiguousarray(X), list(y), dY.astype(np.float32), "sqexp", np.ascontiguousarray(lam),
                                    amp.astype(np.float32), list(sig), sgd, device=2)
    assert ll.tolist() == [-1.0, -2.0, -3.0, -4.0] and st.tolist() == [0, 3, 0, 0]
    assert [type(g) for g in gps] == [api.GradGP] * S and [g._h.value for g in gps] == [1000, 1001, 1002, 1003]
    assert all((g.d, g.n, g.N, g.device, g.kernel) == (d, n, n * (1 + d), 2, api.KERNELS["sqexp"]) for g in gps)
    assert gps[0].logpdf == -1.0 and gps[1].logpdf is None                          # the failed member is an unfitted handle
    name, a = fake.calls[-1]
    assert name == "ggp_fit" and tuple(a[:4]) == (2, api.KERNELS["sqexp"], d, n) and a[7] == S
    assert np.array_equal(a[4], X.reshape(-1, order="F"))
    assert np.array_equal(a[6], dY.astype(np.float32).astype(np.float64).reshape(-1, order="F"))
    assert np.array_equal(a[8], lam.reshape(-1, order="F"))
    assert np.array_equal(a[9], amp.astype(np.float32).astype(np.float64)) and np.array_equal(a[10], sig) and np.array_equal(a[11], sgd)
    n_ok = len(fake.calls)
    for bad in (lambda: api.ggp_fit_batch(X, y, dY, "sqexp", lam[:2], amp, sig, sgd),
                lambda: api.ggp_fit_batch(X, y, dY, "sqexp", lam, amp[:3], sig, sgd),
                lambda: api.ggp_fit_batch(X, y, dY, "sqexp", lam, amp, sig, sgd[:1]),
                lambda: api.ggp_fit_batch(X, y[:4], dY, "sqexp", lam, amp, sig, sgd),
                lambda: api.ggp_fit_batch(X, y, dY[:2], "sqexp", lam, amp, sig, sgd),
                lambda: api.ggp_fit_batch(X, y, dY, "sqexp", lam[:, 0], amp, sig, sgd),
                lambda: api.ggp_fit_batch(X, y, dY, "sqexp", np.zeros((d, 0)), [], [], [])):        # no set: nothing to build
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert len(fake.calls) == n_ok                                                 # none of the refused calls reached the library
    for g in gps:
        g.close()


def test_ngp_fit_batch_and_predict_set_wrappers_check_and_convert(monkeypatch):
    from boss_jl_amd import api
    fake = _FakeLib()
    monkeypatch.setattr(api, "load_library", lambda path=None: fake)
    rng = np.random.default_rng(1)
    d, N, S, M = 2, 6, 3, 5
    fake.d = d
    X, y = rng.uniform(0, 1, (d, N)), rng.standard_normal(N)
    lam, amp, noi = rng.uniform(0.3, 1, (d, N, S)), rng.uniform(0.5, 2, (N, S)), rng.uniform(0.05, 0.3, (N, S))
    m_per = rng.standard_normal((S, N))
    gps, ll, st = api.ngp_fit_batch(X, y, np.ascontiguousarray(lam), amp.astype(np.float32), np.ascontiguousarray(noi),
                                    mean_X=np.asfortranarray(m_per), discrete=[True, False], device=1)
    assert ll.tolist() == [-2.0, -3.0, -4.0] and not st.any()
    assert [type(g) for g in gps] == [api.GibbsGP] * S and all((g.d, g.N, g.device) == (d, N, 1) for g in gps)
    name, a = fake.calls[-1]
    assert name == "ngp_fit" and tuple(a[:3]) == (1, d, N) and a[5].tolist() == [1, 0] and a[6] == S and a[11] == N
    for s in range(S):                                                             # set after set, each d×N column-major
        assert np.array_equal(a[7][s * d * N:(s + 1) * d * N], lam[:, :, s].reshape(-1, order="F"))
    assert np.array_equal(a[8], amp.astype(np.float32).astype(np.float64).reshape(-1, order="F"))
    assert np.array_equal(a[9], noi.reshape(-1, order="F")) and np.array_equal(a[10], m_per.reshape(-1))
    n_ok = len(fake.calls)
    for bad in (lambda: api.ngp_fit_batch(X, y, lam[:, :, 0], amp, noi),
                lambda: api.ngp_fit_batch(X, y, lam, amp.T, noi),
                lambda: api.ngp_fit_batch(X, y, lam, amp, noi[:, :2]),
                lambda: api.ngp_fit_batch(X, y[:-1], lam, amp, noi),
                lambda: api.ngp_fit_batch(X, y, lam, amp, noi, mean_X=m_per[:2]),
                lambda: api.ngp_fit_batch(X, y, lam, amp, noi, discrete=[True]),
                lambda: api.ngp_fit_batch(X, y, np.zeros((d, N, 0)), np.zeros((N, 0)), np.zeros((N, 0)))):
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert len(fake.calls) == n_ok
    # the set prediction: candidates d×M, latent values member after member, prior means one row per member
    Xs = rng.uniform(0, 1, (d, M))
    lam_s, amp_s, ms = rng.uniform(0.3, 1, (d, M, S)), rng.uniform(0.5, 2, (M, S)), rng.standard_normal((S, M))
    mu, var = api.ngp_predict_set(gps, np.ascontiguousarray(Xs), np.ascontiguousarray(lam_s), amp_s.astype(np.float32), np.asfortranarray(ms))
    assert mu.shape == (S, M) and var.shape == (S, M) and mu[1, 2] == 1 * M + 2 and var[2, 0] == 0.5 + 2 * M
    name, a = fake.calls[-1]
    assert name == "ngp_set" and a[0] == S and a[1] == [2000, 2001, 2002] and a[2] == M
    assert np.array_equal(a[3], Xs.reshape(-1, order="F"))
    for s in range(S):
        assert np.array_equal(a[4][s * d * M:(s + 1) * d * M], lam_s[:, :, s].reshape(-1, order="F"))
    assert np.array_equal(a[5], amp_s.astype(np.float32).astype(np.float64).reshape(-1, order="F")) and np.array_equal(a[6], ms.reshape(-1))
    api.ngp_predict_set(gps, Xs, lam_s, amp_s)
    assert fake.calls[-1][1][6] is None
    n_ok = len(fake.calls)
    for bad in (lambda: api.ngp_predict_set(gps, Xs, lam_s[:, :, :2], amp_s),                           # one member short
                lambda: api.ngp_predict_set(gps, Xs, lam_s, amp_s.T),
                lambda: api.ngp_predict_set(gps, Xs[:1], lam_s, amp_s),
                lambda: api.ngp_predict_set(gps, Xs, lam_s, amp_s, ms.T),
                lambda: api.ngp_predict_set(gps[:2], Xs, lam_s, amp_s),
                lambda: api.ngp_predict_set([], Xs, lam_s, amp_s)):
        with pytest.raises((ValueError, api.BossError)):
            bad()
    assert len(fake.calls) == n_ok
    for g in gps:
        g.close()


class _Handle:
    def __init__(self, tag):
        self.tag, self.closed, self.d, self.device = tag, False, 2, 0

    def close(self):
        self.closed = True


def test_gradient_model_posterior_of_a_sample_list_is_one_fit_batch_per_output(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api, gradient_gp
    rng = np.random.default_rng(3)
    d, n, P, S = 2, 6, 2, 5
    data = B.GradientData(rng.uniform(0, 1, (d, n)), rng.standard_normal((P, n)), rng.standard_normal((P, d, n)))
    prm = [B.HipGradientGPParams(rng.uniform(0.4, 0.8, (d, P)), rng.uniform(0.8, 1.4, P), rng.uniform(0.02, 0.06, P),
                                 rng.uniform(0.05, 0.2, P)) for _ in range(S)]
    model = B.HipGradientGaussianProcess([None] * P, [None] * P, [None] * P, [None] * P, kernel="matern32", device=0)
    seen, made = [], []
    fail = {}

    def fake(X, y, dY, kernel, lam, amp, sig, sgd, device=0):
        seen.append((X, y, dY, kernel, lam, amp, sig, sgd, device))
        if fail.get("alloc") == len(seen):
            raise api.BossError(api.BOSS_E_ALLOC, "device allocation failed")
        st = np.zeros(S, dtype=np.int32)
        if fail.get("notpd") == len(seen):
            st[3] = api.BOSS_E_NOT_PD
        hs = [_Handle((len(seen) - 1, s)) for s in range(S)]
        made.extend(hs)
        return hs, np.arange(1.0, S + 1), st
    monkeypatch.setattr(api, "ggp_fit_batch", fake)
    loops = []
    monkeypatch.setattr(B.HipGradientGaussianProcess, "model_posterior_slice",
                        lambda self, p, data_, i: loops.append((id(p), i)) or ("slice", id(p), i))
    assert gradient_gp.batched_call_pays(n * (1 + d), S)
    posts = model.model_posterior(prm, data)
    assert len(seen) == P and not loops and len(posts) == S                         # ONE batched call per output, no create + update loop
    for i, (X, y, dY, kernel, lam, amp, sig, sgd, device) in enumerate(seen):
        assert np.array_equal(X, data.X) and np.array_equal(y, data.Y[i]) and np.array_equal(dY, data.dY[i]) and kernel == "matern32"
        assert np.array_equal(lam, np.stack([p.lengthscales[:, i] for p in prm], axis=1))
        assert amp.tolist() == [p.amplitudes[i] for p in prm] and sig.tolist() == [p.noise_std[i] for p in prm]
        assert sgd.tolist() == [p.grad_noise_std[i] for p in prm]
    for s, post in enumerate(posts):                                                # posts[s] holds output i's member s
        assert [sl.gp.tag for sl in post.slices] == [(i, s) for i in range(P)] and all(sl.params is prm[s] for sl in post.slices)
    # a sample that is not PD raises as the loop does, and nothing stays resident
    seen.clear(), made.clear()
    fail["notpd"] = 2
    with pytest.raises(api.PosDefException):
        model.model_posterior(prm, data)
    assert len(made) == 2 * S and all(h.closed for h in made)
    # a batch that does not fit the device: what was built is released and the loop takes over
    seen.clear(), made.clear(), fail.clear()
    fail["alloc"] = 2
    posts = model.model_posterior(prm, data)
    assert len(seen) == 2 and all(h.closed for h in made) and len(loops) == S * P and len(posts) == S
    # where a batch does not pay, the loop runs and the batch entry point is not called
    seen.clear(), loops.clear(), fail.clear()
    monkeypatch.setattr(gradient_gp, "batched_call_pays", lambda rows, n_sets: False)
    posts = model.model_posterior(prm, data)
    assert not seen and len(loops) == S * P and len(posts) == S
    assert model.model_posterior([], data) == []


def test_nonstationary_posterior_batch_and_averaged_acquisition(monkeypatch):
    """λ(·), α(·) at the ROUNDED points, σ(·) and the prior mean at the points as given, for every model — one boss_ngp_fit_batch per
    output; the averaged acquisition is one set prediction per output and one moments call."""
    import boss_jl_amd as B
    from boss_jl_amd import api, nonstationary
    rng = np.random.default_rng(2)
    d, N, P, S, M = 2, 7, 2, 3, 4
    X = rng.uniform(0, 4, (d, N))
    data = B.ExperimentData(X, rng.standard_normal((P, N)))
    disc = [False, True]

    def model(c):
        return B.HipNonstationaryGP(f_lam=[lambda x, c=c: c * (0.3 + 0.1 * np.asarray(x) ** 2)] * P, f_amp=[lambda x, c=c: 1.0 + c * x[1]] * P,
                                    f_noise=[lambda x, c=c: 0.1 * c + 0.01 * x[1]] * P,
                                    mean=None if c == 2.0 else [lambda x, c=c: c * x[1], None], discrete=disc)
    models = [model(c) for c in (1.0, 2.0, 3.0)]
    seen, made = [], []
    notpd = {}

    def fake(Xa, y, lam, amp, noi, mean_X=None, discrete=None, device=0):
        seen.append((Xa, y, lam.copy(), amp.copy(), noi.copy(), mean_X, discrete, device))
        st = np.zeros(S, dtype=np.int32)
        if notpd.get("at") == len(seen):
            st[2] = api.BOSS_E_NOT_PD
        hs = [_Handle((len(seen) - 1, s)) for s in range(S)]
        made.extend(hs)
        return hs, np.array([1.0, 2.0, 3.0]), st
    monkeypatch.setattr(api, "ngp_fit_batch", fake)
    posts = nonstationary.nonstationary_model_posterior_batch(models, data)
    assert len(seen) == P and len(posts) == S and all(len(r) == P for r in posts)    # ONE batched call per output
    for i, (Xa, y, lam, amp, noi, mean_X, discrete, device) in enumerate(seen):
        assert np.array_equal(Xa, X) and np.array_equal(y, data.Y[i]) and list(discrete) == disc and device == 0
        for s, m in enumerate(models):
            l1, a1, n1, m1, _ = m._latent_at_data(X, i)
            assert np.array_equal(lam[:, :, s], l1) and np.array_equal(amp[:, s], a1) and np.array_equal(noi[:, s], n1)
        if i == 0:
            assert mean_X.shape == (S, N) and np.array_equal(mean_X[0], X[1]) and not mean_X[1].any() and np.array_equal(mean_X[2], 3.0 * X[1])
        else:
            assert mean_X is None
    for s in range(S):
        for i in range(P):
            sl = posts[s][i]
            assert sl.gp.tag == (i, s) and sl.f_lam is models[s].f_lam[i] and sl.f_noise is models[s].f_noise[i]
            assert sl.mean_fn is (None if models[s].mean is None else models[s].mean[i]) and list(sl.discrete) == disc
    # averaged acquisition: per output one set prediction over the S members, with every sample's latent values at the rounded candidates
    Xs = rng.uniform(0, 4, (d, M))
    Xr = Xs.copy()
    Xr[1] = np.rint(Xr[1])
    sets, mom = [], []

    def fake_set(gps, Xa, lam, amp, mean_Xs=None):
        sets.append((list(gps), Xa, lam.copy(), amp.copy(), mean_Xs))
        k = len(sets)
        return np.full((S, M), 1.0 * k) + np.arange(S)[:, None], np.full((S, M), 0.1 * k)

    def fake_mom(mu, var, fit_coefs, y_max=None, best=None, valid_mask=None, device=0):
        mom.append((mu.copy(), var.copy(), fit_coefs, y_max, best, valid_mask, device))
        return np.zeros(M), 1, 0.25
    monkeypatch.setattr(api, "ngp_predict_set", fake_set)
    monkeypatch.setattr(api, "acq_ei_moments", fake_mom)
    mask = np.array([True, False, True, True])
    out = nonstationary.nonstationary_acq_ei_batch(posts, Xs, [1.0, 0.0], [np.inf, 0.3], 0.7, valid_mask=mask)
    assert out[1:] == (1, 0.25) and len(sets) == P and len(mom) == 1
    for i, (gps, Xa, lam, amp, mean_Xs) in enumerate(sets):
        assert [g.tag for g in gps] == [(i, s) for s in range(S)] and np.array_equal(Xa, Xs)
        for s, c in enumerate((1.0, 2.0, 3.0)):
            assert np.allclose(lam[:, :, s], c * (0.3 + 0.1 * Xr ** 2), rtol=0, atol=0) and np.array_equal(amp[:, s], 1.0 + c * Xr[1])
        if i == 0:                                              # the prior mean sees the candidates as given
            assert np.array_equal(mean_Xs[0], Xs[1]) and not mean_Xs[1].any() and np.array_equal(mean_Xs[2], 3.0 * Xs[1])
        else:
            assert mean_Xs is None
    mu, var, coefs, y_max, best, vm, device = mom[0]
    assert mu.shape == (S, P, M) and np.array_equal(mu[:, 1, 0], 2.0 + np.arange(S)) and np.array_equal(var[:, 0, :], np.full((S, M), 0.1))
    assert coefs == [1.0, 0.0] and y_max == [np.inf, 0.3] and best == 0.7 and vm is mask
    # a sample that is not PD raises and releases what was built; mismatched models are refused
    seen.clear(), made.clear()
    notpd["at"] = 2
    with pytest.raises(api.PosDefException):
        nonstationary.nonstationary_model_posterior_batch(models, data)
    assert len(made) == 2 * S and all(h.closed for h in made)
    assert nonstationary.nonstationary_model_posterior_batch([], data) == []
    with pytest.raises(ValueError):
        nonstationary.nonstationary_model_posterior_batch([models[0], B.HipNonstationaryGP(models[0].f_lam, models[0].f_amp, models[0].f_noise)], data)
    assert B.nonstationary_model_posterior_batch is nonstationary.nonstationary_model_posterior_batch
    assert B.nonstationary_acq_ei_batch is nonstationary.nonstationary_acq_ei_batch
    assert callable(B.ggp_fit_batch) and callable(B.ngp_fit_batch) and callable(B.ngp_predict_set)
