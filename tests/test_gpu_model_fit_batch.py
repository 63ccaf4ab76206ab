"""boss_ggp_fit_batch / boss_ngp_fit_batch and the one-launch prediction of their members (pytest -m gpu).

The reference builds one posterior per hyper-parameter sample for every model (/root/reference/src/posterior.jl:15-19) and averages
the acquisition over them (/root/reference/src/acquisitions/expected_improvement.jl:87-90).  Here the S posteriors of a
gradient-observation or a nonstationary output come out of ONE batched factorisation as resident handles, boss_acq_ei walks
gradient-model members in one prediction launch and boss_ngp_predict_set does the same for nonstationary members.

Tolerances are the project's own for these quantities (tests/test_gpu_fit_batch.py, tests/test_gpu_model_batch.py):
|Δμ| <= 1e-9 (1 + max|μ|), |Δσ²| <= 1e-9 α² + 1e-12 (nonstationary: the largest α(x*)²), |ΔL| <= 1e-9 (1 + max|L|),
set against loop 1e-12 absolute, acquisition against the oracle 1e-10 absolute; log-likelihoods and factors bitwise against the
likelihood batch and single updates.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


# ------------------------------------------------------------------------------------------ cases
def grad_case(n, d, S, seed=0):
    """y = sin(Xᵀw) with its exact gradient; S draws λ ∈ [0.3, 1.5], α ∈ [0.5, 2], σ, σ_∂ ∈ [0.05, 0.3] (tests/test_gpu_model_batch.py)."""
    rng = np.random.default_rng(100 + seed)
    X = rng.uniform(0, 1, (d, n))
    w = rng.uniform(0.5, 2.0, d)
    y = np.sin(X.T @ w)
    dY = w[:, None] * np.cos(X.T @ w)[None, :]
    lam = rng.uniform(0.3, 1.5, (d, S))
    amp, sig, sgd = rng.uniform(0.5, 2.0, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.05, 0.3, S)
    return X, y, dY, lam, amp, sig, sgd


def latent(d):
    f_lam = lambda x: 0.25 + 0.5 * np.asarray(x) ** 2 + 0.1 * np.arange(1, d + 1)        # noqa: E731
    f_amp = lambda x: 1.0 + 0.4 * np.sin(3 * x[0])                                        # noqa: E731
    f_noise = lambda x: 0.03 + 0.05 * x[-1] ** 2                                           # noqa: E731
    return f_lam, f_amp, f_noise


def ev(f, Z, scale=1.0):
    return np.array([f(Z[:, j] / scale) for j in range(Z.shape[1])])


def ns_case(d, N, S, M, seed=4, disc=None):
    """Data on [0, scale]^d (scale 3 with discrete dimensions, so that rounding matters), S sets of the latent family scaled by
    c ∈ [0.7, 1.6] (λ), a ∈ [0.6, 1.8] (α), n ∈ [1, 3] (σ), and the same family at M candidates."""
    rng = np.random.default_rng(seed)
    scale = 1.0 if disc is None else 3.0
    X = rng.uniform(0, scale, (d, N))
    y = np.sin(2 * np.pi * X / scale).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    Xs = rng.uniform(0, scale, (d, M))

    def rounded(Z):
        Zr = Z.copy()
        if disc is not None:
            Zr[np.asarray(disc, bool)] = np.rint(Zr[np.asarray(disc, bool)])
        return Zr
    f_lam, f_amp, f_noise = latent(d)
    r2 = np.random.default_rng(seed + 50)
    c, a, nz = r2.uniform(0.7, 1.6, S), r2.uniform(0.6, 1.8, S), r2.uniform(1.0, 3.0, S)
    lam = np.asfortranarray(ev(f_lam, rounded(X), scale).T[:, :, None] * c[None, None, :])
    amp = np.asfortranarray(ev(f_amp, rounded(X), scale)[:, None] * a[None, :])
    noi = np.asfortranarray(ev(f_noise, X, scale)[:, None] * nz[None, :])
    lam_s = np.asfortranarray(ev(f_lam, rounded(Xs), scale).T[:, :, None] * c[None, None, :])
    amp_s = np.asfortranarray(ev(f_amp, rounded(Xs), scale)[:, None] * a[None, :])
    return X, y, lam, amp, noi, Xs, lam_s, amp_s


def ei_from_moments(O, mus, vars_, coefs, y_max, best, mask):
    """construct_ei + the BI average (expected_improvement.jl:68-90) from oracle moments mus[s], vars_[s] of shape P×M."""
    acc = np.zeros(mus[0].shape[1])
    for mu, var in zip(mus, vars_):
        if best is None:
            acc += O.feas_prob(mu, var, y_max)
        elif y_max is None:
            acc += O.expected_improvement_lin(coefs, mu, var, best)
        else:
            acc += O.expected_improvement_lin(coefs, mu, var, best) * O.feas_prob(mu, var, y_max)
    acq = acc / len(mus)
    return acq if mask is None else np.where(mask, acq, 0.0)


def close_all(gps, order_seed=0):
    for s in np.random.default_rng(order_seed).permutation(len(gps)):   # any order; the shared storage goes with the last one
        gps[s].close()


# ------------------------------------------------------------------------------------------ 1. members against the oracle, bitwise agreement
# rows n (1 + d): 240 and 260 (either side of one 256-row block), 2043 and 2061 (either side of 2048)
GRAD_SHAPES = [("matern32", 120, 1, 5), ("matern52", 65, 3, 33), ("sqexp", 227, 8, 2), ("matern52", 229, 8, 2), ("sqexp", 30, 3, 5)]


@pytest.mark.parametrize("kernel,n,d,S", GRAD_SHAPES)
def test_gradient_members_match_oracle_and_single_handles(api, O, kernel, n, d, S):
    X, y, dY, lam, amp, sig, sgd = grad_case(n, d, S, seed=n)
    Xs = np.random.default_rng(n).uniform(0, 1, (d, 45))
    gps, ll, st = api.ggp_fit_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    assert not st.any() and np.isfinite(ll).all()
    ll_b, st_b = api.ggp_loglike_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    single = api.GradGP(X, y, dY, kernel)
    checked = range(S) if S <= 5 else (0, S // 2, S - 1)       # (the oracle builds its matrices in Python loops)
    for s in range(S):
        lp = single.update(lam[:, s], amp[s], sig[s], sgd[s])
        print(f"[fit-batch] ggp {kernel} n={n} d={d} set {s}: fit {ll[s]!r} batch {ll_b[s]!r} single {lp!r}")
        assert ll[s] == ll_b[s] and ll[s] == lp, (s, ll[s], ll_b[s], lp)
        L, z = gps[s].factor()
        L1, z1 = single.factor()
        dL = float(np.abs(np.tril(L) - np.tril(L1)).max())
        print(f"[fit-batch] ggp set {s}: max |L - L_single| {dL:.3e}")
        assert np.array_equal(np.tril(L), np.tril(L1)) and np.array_equal(z, z1), (s, dL)
        if s not in checked:
            continue
        post = O.gradient_gp_fit(X, y, dY, kernel, lam[:, s], amp[s], sig[s], sgd[s])
        mu, var = gps[s].predict(Xs)
        mu_o, var_o = O.gradient_gp_mean_and_var(post, Xs)
        assert np.allclose(mu, mu_o, rtol=0, atol=1e-9 * (1 + np.abs(mu_o).max())), s
        assert np.allclose(var, var_o, rtol=0, atol=1e-9 * amp[s] ** 2 + 1e-12), s
        assert np.allclose(np.tril(L), post.L, rtol=0, atol=1e-9 * (1 + np.abs(post.L).max())), s
    single.close()
    close_all(gps, n)


NS_SHAPES = [(1, 250, 5, None, None), (3, 260, 33, None, "shared"), (8, 2040, 2, None, None), (3, 2060, 2, None, "per"),
             (3, 150, 5, [False, True, False], "per")]


@pytest.mark.parametrize("d,N,S,disc,mean", NS_SHAPES)
def test_nonstationary_members_match_oracle_and_single_handles(api, O, d, N, S, disc, mean):
    M = 45
    X, y, lam, amp, noi, Xs, lam_s, amp_s = ns_case(d, N, S, M, seed=N, disc=disc)
    rng = np.random.default_rng(N)
    th = rng.standard_normal((S, d + 1)) * 0.1
    mfn = (lambda s, Z: th[0, 0] + th[0, 1:] @ Z) if mean == "shared" else (lambda s, Z: th[s, 0] + th[s, 1:] @ Z)
    mX = None if mean is None else (mfn(0, X) if mean == "shared" else np.stack([mfn(s, X) for s in range(S)]))
    gps, ll, st = api.ngp_fit_batch(X, y, lam, amp, noi, mean_X=mX, discrete=disc)
    assert not st.any() and np.isfinite(ll).all()
    ll_b, st_b = api.ngp_loglike_batch(X, y, lam, amp, noi, mean_X=mX, discrete=disc)
    single = api.GibbsGP(X, y, disc)
    checked = range(S) if S <= 5 else (0, S // 2, S - 1)
    for s in range(S):
        m_s = None if mean is None else mfn(s, X)
        lp = single.update(lam[:, :, s], amp[:, s], noi[:, s], m_s)
        print(f"[fit-batch] ngp d={d} N={N} set {s}: fit {ll[s]!r} batch {ll_b[s]!r} single {lp!r}")
        assert ll[s] == ll_b[s] and ll[s] == lp, (s, ll[s], ll_b[s], lp)
        L, z = gps[s].factor()
        L1, z1 = single.factor()
        dL = float(np.abs(np.tril(L) - np.tril(L1)).max())
        print(f"[fit-batch] ngp set {s}: max |L - L_single| {dL:.3e}")
        assert np.array_equal(np.tril(L), np.tril(L1)) and np.array_equal(z, z1), (s, dL)
        if s not in checked:
            continue
        post = O.nonstationary_fit(X, y, lam[:, :, s], amp[:, s], noi[:, s], mean=m_s, discrete=disc)
        ms = None if mean is None else mfn(s, Xs)
        mu, var = gps[s].predict(Xs, lam_s[:, :, s], amp_s[:, s], ms)
        mu_o, var_o = O.nonstationary_mean_and_var(post, Xs, lam_s[:, :, s], amp_s[:, s], mean_s=ms)
        assert np.allclose(mu, mu_o, rtol=0, atol=1e-9 * (1 + np.abs(mu_o).max())), s
        assert np.allclose(var, var_o, rtol=0, atol=1e-9 * (amp_s[:, s] ** 2).max() + 1e-12), s
        assert np.allclose(np.tril(L), post.L, rtol=0, atol=1e-9 * (1 + np.abs(post.L).max())), s
    single.close()
    close_all(gps, N)


# ------------------------------------------------------------------------------------------ 2. set prediction
@pytest.mark.parametrize("P,n,d,S,M,y_max,with_best,with_mask", [(1, 30, 3, 5, 70, None, True, False), (2, 65, 3, 4, 33, [np.inf, 0.3], True, True),
                                                              (2, 120, 1, 3, 257, [0.9, 0.3], False, True), (1, 227, 8, 2, 50, [0.5], True, False)])
def test_gradient_set_prediction_matches_loop_and_oracle(api, O, P, n, d, S, M, y_max, with_best, with_mask):
    """EI × feasibility averaged over the S members of P outputs through boss_acq_ei: the set path must be taken (launch counter),
    agree with the member-by-member loop on the same handles (moments through each member's own predict, then the moments
    epilogue) and with the oracle."""
    kernel = "matern52"
    cases = [grad_case(n, d, S, seed=10 * n + p) for p in range(P)]
    X = cases[0][0]
    Xs = np.random.default_rng(n + 7).uniform(0, 1, (d, M))
    gps = []
    for p in range(P):
        _, y, dY, lam, amp, sig, sgd = cases[p]
        g, ll, st = api.ggp_fit_batch(X, y, dY, kernel, lam, amp, sig, sgd)
        assert not st.any()
        gps.append(g)
    handles = [[gps[p][s] for p in range(P)] for s in range(S)]
    coefs = [1.0, 0.0][:P]
    best = float(cases[0][1].max()) if with_best else None
    mask = (np.random.default_rng(1).uniform(size=M) > 0.1) if with_mask else None
    before = api._set_launches()
    acq, am, mx = api.acq_ei(handles, api.Candidates(Xs), coefs, y_max, best, valid_mask=mask)
    after = api._set_launches()
    assert after[1] > before[1], "boss_acq_ei over gradient-model members did not take the set prediction"
    mu_l = np.array([[gps[p][s].predict(Xs)[0] for p in range(P)] for s in range(S)])
    var_l = np.array([[gps[p][s].predict(Xs)[1] for p in range(P)] for s in range(S)])
    loop, _, _ = api.acq_ei_moments(mu_l, var_l, coefs, y_max, best, valid_mask=mask)
    print(f"[fit-batch] ggp set vs loop: max |d| {np.abs(acq - loop).max():.3e}")
    assert np.allclose(acq, loop, rtol=0, atol=1e-12), float(np.abs(acq - loop).max())
    mus, vars_ = [], []
    for s in range(S):
        mv = [O.gradient_gp_mean_and_var(O.gradient_gp_fit(X, cases[p][1], cases[p][2], kernel, cases[p][3][:, s], cases[p][4][s],
                                                            cases[p][5][s], cases[p][6][s]), Xs) for p in range(P)]
        mus.append(np.stack([m[0] for m in mv]))
        vars_.append(np.stack([m[1] for m in mv]))
    want = ei_from_moments(O, mus, vars_, coefs, y_max, best, mask)
    print(f"[fit-batch] ggp set vs oracle: max |d| {np.abs(acq - want).max():.3e}")
    assert np.allclose(acq, want, rtol=0, atol=1e-10), float(np.abs(acq - want).max())
    assert am == int(np.argmax(acq)) and mx == acq[am]
    for row in gps:
        close_all(row)


@pytest.mark.parametrize("P,d,N,S,M,disc,mean,y_max,with_best,with_mask",
                         [(1, 3, 150, 5, 70, None, False, None, True, False), (2, 3, 260, 4, 33, [False, True, False], True, [np.inf, 0.3], True, True),
                          (2, 1, 250, 3, 257, None, True, [0.9, 0.3], False, True), (1, 8, 1100, 2, 50, None, False, [0.5], True, False)])
def test_nonstationary_set_prediction_matches_loop_and_oracle(api, O, P, d, N, S, M, disc, mean, y_max, with_best, with_mask):
    # the outputs share the points; output p has its own observations and the latent family scaled by 1 + p/10 (λ), 1 + p/20 (α)
    X, y0, lam0, amp0, noi0, Xs, lam_s0, amp_s0 = ns_case(d, N, S, M, seed=10 * N, disc=disc)
    y1 = np.cos(2 * np.pi * X / (1.0 if disc is None else 3.0)).sum(0) / np.sqrt(d) + 0.05 * np.random.default_rng(N + 1).standard_normal(N)
    cases = [(X, (y0, y1)[p], np.asfortranarray(lam0 * (1 + 0.1 * p)), np.asfortranarray(amp0 * (1 + 0.05 * p)), noi0, Xs,
              np.asfortranarray(lam_s0 * (1 + 0.1 * p)), np.asfortranarray(amp_s0 * (1 + 0.05 * p))) for p in range(P)]
    rng = np.random.default_rng(N)
    th = rng.standard_normal((S, P, d + 1)) * 0.1
    mfn = lambda s, p, Z: th[s, p, 0] + th[s, p, 1:] @ Z                                  # noqa: E731
    gps = []
    for p in range(P):
        _, y, lam, amp, noi, _, _, _ = cases[p]
        mX = np.stack([mfn(s, p, X) for s in range(S)]) if mean else None
        g, ll, st = api.ngp_fit_batch(X, y, lam, amp, noi, mean_X=mX, discrete=disc)
        assert not st.any()
        gps.append(g)
    coefs = [1.0, 0.0][:P]
    best = float(cases[0][1].max()) if with_best else None
    mask = (np.random.default_rng(1).uniform(size=M) > 0.1) if with_mask else None
    mu = np.empty((S, P, M))
    var = np.empty((S, P, M))
    mus, vars_ = [np.empty((P, M)) for _ in range(S)], [np.empty((P, M)) for _ in range(S)]
    for p in range(P):
        _, y, lam, amp, noi, _, lam_s, amp_s = cases[p]
        ms = np.stack([mfn(s, p, Xs) for s in range(S)]) if mean else None
        before = api._set_launches()
        mu[:, p, :], var[:, p, :] = api.ngp_predict_set(gps[p], Xs, lam_s, amp_s, ms)
        assert api._set_launches()[1] > before[1], "boss_ngp_predict_set over the members of one fit did not take the set prediction"
        for s in range(S):
            m1, v1 = gps[p][s].predict(Xs, lam_s[:, :, s], amp_s[:, s], None if ms is None else ms[s])
            assert np.allclose(mu[s, p], m1, rtol=0, atol=1e-12) and np.allclose(var[s, p], v1, rtol=0, atol=1e-12), \
                (p, s, float(np.abs(mu[s, p] - m1).max()), float(np.abs(var[s, p] - v1).max()))
            post = O.nonstationary_fit(X, y, lam[:, :, s], amp[:, s], noi[:, s], mean=mfn(s, p, X) if mean else None, discrete=disc)
            mus[s][p], vars_[s][p] = O.nonstationary_mean_and_var(post, Xs, lam_s[:, :, s], amp_s[:, s], mean_s=None if ms is None else ms[s])
            assert np.allclose(mu[s, p], mus[s][p], rtol=0, atol=1e-9 * (1 + np.abs(mus[s][p]).max()))
            assert np.allclose(var[s, p], vars_[s][p], rtol=0, atol=1e-9 * (amp_s[:, s] ** 2).max() + 1e-12)
    acq, am, mx = api.acq_ei_moments(mu, var, coefs, y_max, best, valid_mask=mask)
    want = ei_from_moments(O, mus, vars_, coefs, y_max, best, mask)
    print(f"[fit-batch] ngp set vs oracle: max |d| {np.abs(acq - want).max():.3e}")
    assert np.allclose(acq, want, rtol=0, atol=1e-10), float(np.abs(acq - want).max())
    assert am == int(np.argmax(acq)) and mx == acq[am]
    # a list that is not uniform (here: a handle on one observation less) is predicted member by member inside the same call
    lone = api.GibbsGP(X[:, :-1], cases[0][1][:-1], disc)
    lone.update(cases[0][2][:, :-1, 0], cases[0][3][:-1, 0], cases[0][4][:-1, 0], mfn(0, 0, X[:, :-1]) if mean else None)
    before = api._set_launches()
    ms0 = np.stack([mfn(0, 0, Xs), mfn(1, 0, Xs)]) if mean else None
    mu2, var2 = api.ngp_predict_set([lone, gps[0][1]], Xs, cases[0][6][:, :, :2], cases[0][7][:, :2], ms0)
    assert api._set_launches() == before
    m1, v1 = lone.predict(Xs, cases[0][6][:, :, 0], cases[0][7][:, 0], None if ms0 is None else ms0[0])
    assert np.allclose(mu2[0], m1, rtol=0, atol=1e-12) and np.allclose(var2[0], v1, rtol=0, atol=1e-12)
    assert np.allclose(mu2[1], mu[1, 0], rtol=0, atol=1e-12) and np.allclose(var2[1], var[1, 0], rtol=0, atol=1e-12)
    lone.close()
    for row in gps:
        close_all(row)


def test_nonstationary_set_prediction_domain_error(api, O):
    """Well-separated points, a huge amplitude and a tiny noise, predicted at the training points (test_nonstationary_cov_domain_error):
    the variance of that member falls below −1e-8; the set call raises what the member's own predict raises, with its bad_index."""
    X = np.arange(0.0, 400.0, 10.0)[None, :]
    y = np.sin(X[0])
    N = X.shape[1]
    lam = np.asfortranarray(np.full((1, N, 3), 3.0))
    amp = np.asfortranarray(np.stack([np.full(N, 1.0), np.full(N, 1e5), np.full(N, 1e5)], axis=1))
    noi = np.asfortranarray(np.stack([np.full(N, 0.1), np.full(N, 1e-4), np.full(N, 1e-4)], axis=1))
    gps, ll, st = api.ngp_fit_batch(X, y, lam, amp, noi)
    assert not st.any()
    mu0, var0 = gps[0].predict(X, lam[:, :, 0], amp[:, 0])
    with pytest.raises(api.DomainError) as e1:
        gps[1].predict(X, lam[:, :, 1], amp[:, 1])
    with pytest.raises(api.DomainError) as e:
        api.ngp_predict_set(gps, X, lam, amp)
    assert e.value.code == api.BOSS_E_NEG_VAR and e.value.bad_index == e1.value.bad_index and 0 <= e.value.bad_index < N
    mu, var = api.ngp_predict_set(gps[:1] + gps[:1], X, lam[:, :, [0, 0]], amp[:, [0, 0]])       # the healthy member alone is fine
    assert np.allclose(mu[0], mu0, rtol=0, atol=1e-12) and np.allclose(var[1], var0, rtol=0, atol=1e-12)
    close_all(gps)


# ------------------------------------------------------------------------------------------ 3. members as ordinary handles, failures, storage
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from boss_jl_amd import api
from oracle import gp_oracle as O
import test_gpu_model_fit_batch as T

def same(a, b, what, tol=1e-9):
    a, b = np.asarray(a), np.asarray(b)
    assert np.allclose(a, b, rtol=0, atol=tol * (1 + np.abs(b).max())), (what, float(np.abs(a - b).max()))

# ---- gradient-observation members
n, d, S, kernel = 65, 3, 6, "matern52"
X, y, dY, lam, amp, sig, sgd = T.grad_case(n, d, S, seed=3)
Xs = np.random.default_rng(5).uniform(0, 1, (d, 40))
def fresh_g(s, Xd=X, yd=y, dYd=dY, par=None):
    g = api.GradGP(Xd, yd, dYd, kernel)
    p = par or (lam[:, s], amp[s], sig[s], sgd[s])
    g.update(*p)
    return g
def check_g(g, ref):
    for a, b, w in zip(g.predict(Xs), ref.predict(Xs), ("mu", "var")): same(a, b, w)
for rnd in range(2):                                            # the second fit reuses the storage the first one released
    gps, ll, st = api.ggp_fit_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    assert not st.any()
    refs = [fresh_g(s) for s in range(S)]
    for s in range(S):
        check_g(gps[s], refs[s])
        for a, b, w in zip(gps[s].predict_grad(Xs), refs[s].predict_grad(Xs), ("mu", "var", "dmu", "dvar")): same(a, b, "ggp grad " + w)
        for a, b, w in zip(gps[s].predict_value_cov(Xs), refs[s].predict_value_cov(Xs), ("mu", "cov")): same(a, b, "ggp cov " + w)
        (l0, g0), (l1, g1) = gps[s].loglike_grad(), refs[s].loglike_grad()
        same(l0, l1, "ggp logpdf"); same(g0, g1, "ggp loglike_grad")
    # re-update of member 1 in place, append to member 3 (rebuilt on storage of its own), the siblings keep their factors
    par = (lam[:, 0] * 1.1, 0.9, 0.07, 0.12)
    lp = gps[1].update(*par); r = fresh_g(1, par=par); same(lp, r.logpdf, "ggp re-update"); check_g(gps[1], r); r.close()
    xn = np.random.default_rng(8).uniform(0, 1, (d, 2)); yn = np.array([0.3, -0.2]); dn = np.random.default_rng(9).standard_normal((d, 2))
    lp = gps[3].append(xn, yn, dn)
    r = fresh_g(3, np.concatenate([X, xn], 1), np.concatenate([y, yn]), np.concatenate([dY, dn], 1))
    assert abs(lp - r.logpdf) <= 1e-9 * (1 + abs(r.logpdf)); check_g(gps[3], r); r.close()
    for s in (0, 2, 4, 5): check_g(gps[s], refs[s])
    for s in (4, 0, 3): gps[s].close()                          # shuffled frees; the rest still predicts
    for s in (2, 5): check_g(gps[s], refs[s])
    for s in (5, 1, 2): gps[s].close()
    for r in refs: r.close()

# ---- nonstationary members (a prior mean per set, a discrete dimension)
d, N, S, M = 3, 300, 6, 40
disc = [False, True, False]
X, y, lam, amp, noi, Xs, lam_s, amp_s = T.ns_case(d, N, S, M, seed=11, disc=disc)
th = np.random.default_rng(2).standard_normal((S, d + 1)) * 0.1
mfn = lambda s, Z: th[s, 0] + th[s, 1:] @ Z
mX = np.stack([mfn(s, X) for s in range(S)])
def fresh_n(s, Xd=X, yd=y, l=None, a=None, nz=None, m=None):
    g = api.GibbsGP(Xd, yd, disc)
    g.update(lam[:, :, s] if l is None else l, amp[:, s] if a is None else a, noi[:, s] if nz is None else nz, mX[s] if m is None else m)
    return g
def check_n(g, ref, s):
    for a, b, w in zip(g.predict(Xs, lam_s[:, :, s], amp_s[:, s], mfn(s, Xs)), ref.predict(Xs, lam_s[:, :, s], amp_s[:, s], mfn(s, Xs)), ("mu", "var")):
        same(a, b, "ngp " + w)
for rnd in range(2):
    gps, ll, st = api.ngp_fit_batch(X, y, lam, amp, noi, mean_X=mX, discrete=disc)
    assert not st.any()
    refs = [fresh_n(s) for s in range(S)]
    for s in range(S):
        check_n(gps[s], refs[s], s)
        a4 = gps[s].predict_grad(Xs, lam_s[:, :, s], amp_s[:, s], np.zeros((d, d, M)), np.zeros((d, M)), mfn(s, Xs))
        b4 = refs[s].predict_grad(Xs, lam_s[:, :, s], amp_s[:, s], np.zeros((d, d, M)), np.zeros((d, M)), mfn(s, Xs))
        for a, b, w in zip(a4, b4, ("mu", "var", "dmu", "dvar")): same(a, b, "ngp grad " + w)
        for a, b, w in zip(gps[s].predict_cov(Xs, lam_s[:, :, s], amp_s[:, s], mfn(s, Xs)), refs[s].predict_cov(Xs, lam_s[:, :, s], amp_s[:, s], mfn(s, Xs)), ("mu", "cov")):
            same(a, b, "ngp cov " + w)
        g0, g1 = gps[s].loglike_grad(), refs[s].loglike_grad()
        same(g0[0], g1[0], "ngp logpdf")
        for a, b in zip(g0[1:], g1[1:]): same(a, b, "ngp loglike_grad")
    lp = gps[1].update(lam[:, :, 0] * 1.1, amp[:, 0], noi[:, 0] * 1.5, mX[1])
    r = fresh_n(1, l=lam[:, :, 0] * 1.1, a=amp[:, 0], nz=noi[:, 0] * 1.5); same(lp, r.logpdf, "ngp re-update logpdf")
    for a, b in zip(gps[1].predict(Xs, lam_s[:, :, 0] * 1.1, amp_s[:, 0], mfn(1, Xs)), r.predict(Xs, lam_s[:, :, 0] * 1.1, amp_s[:, 0], mfn(1, Xs))): same(a, b, "ngp re-update")
    r.close()
    xn = np.random.default_rng(8).uniform(0, 3, (d, 2)); yn = np.array([0.3, -0.2])
    xn = X[:, [10, 20]].copy(); xn[0] += 0.01                   # beside two data points, with those points' latent values
    ln, an, nn, mn = lam[:, [10, 20], 3], amp[[10, 20], 3], noi[[10, 20], 3], mfn(3, xn)
    lp = gps[3].append(xn, yn, ln, an, nn, mn)
    r = api.GibbsGP(np.concatenate([X, xn], 1), np.concatenate([y, yn]), disc)
    r.update(np.concatenate([lam[:, :, 3], ln], 1), np.concatenate([amp[:, 3], an]), np.concatenate([noi[:, 3], nn]), np.concatenate([mX[3], mn]))
    assert abs(lp - r.logpdf) <= 1e-9 * (1 + abs(r.logpdf)); check_n(gps[3], r, 3); r.close()
    y2 = y + 0.1; gps[4].set_y(y2); gps[4].update(lam[:, :, 4], amp[:, 4], noi[:, 4], mX[4])   # new observations for member 4 alone
    r = fresh_n(4, yd=y2); check_n(gps[4], r, 4); r.close()
    for s in (0, 2, 5): check_n(gps[s], refs[s], s)
    # the members that are still views of the slab predict together, the others through their own path, in one call
    mu, var = api.ngp_predict_set([gps[0], gps[2], gps[5]], Xs, lam_s[:, :, [0, 2, 5]], amp_s[:, [0, 2, 5]], np.stack([mfn(s, Xs) for s in (0, 2, 5)]))
    for k, s in enumerate((0, 2, 5)):
        m1, v1 = refs[s].predict(Xs, lam_s[:, :, s], amp_s[:, s], mfn(s, Xs)); same(mu[k], m1, "set mu"); same(var[k], v1, "set var")
    for s in (4, 0, 3): gps[s].close()
    for s in (2, 5): check_n(gps[s], refs[s], s)
    for s in (5, 1, 2): gps[s].close()
    for r in refs: r.close()
print("RES ok")
'''


def test_members_are_ordinary_handles_on_poisoned_allocations(api):
    """predict_grad, the covariances, loglike_grad, a re-update, an append, new observations and frees in shuffled order on members
    of both models, each against a fresh single handle; two fits in a row; every fresh device block filled with NaN patterns
    (BOSS_POISON_ALLOC=1, a child process) so that nothing passes on memory the batch kernels never wrote."""
    code = CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BOSS_POISON_ALLOC="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "RES ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_failures_stay_local(api):
    """A set with a negative parameter and one whose matrix is not PD (a duplicated point, zero noise) are reported per set; their
    neighbours are bit-identical to a batch without them; predict on a failed member is BOSS_E_NOT_FITTED."""
    n, d, S, kernel = 40, 2, 5, "sqexp"
    X, y, dY, lam, amp, sig, sgd = grad_case(n, d, S, seed=1)
    X[:, 1] = X[:, 0]
    Xs = np.random.default_rng(0).uniform(0, 1, (d, 33))
    amp2, sig2, sgd2 = amp.copy(), sig.copy(), sgd.copy()
    amp2[1] = -1.0                                                # invalid
    sig2[3] = sgd2[3] = 0.0                                       # two coincident points without noise: not PD
    gps, ll, st = api.ggp_fit_batch(X, y, dY, kernel, lam, amp2, sig2, sgd2)
    assert st.tolist() == [0, api.BOSS_E_INVALID, 0, api.BOSS_E_NOT_PD, 0] and ll[1] == -np.inf and ll[3] == -np.inf
    keep = [0, 2, 4]
    gk, llk, stk = api.ggp_fit_batch(X, y, dY, kernel, lam[:, keep], amp[keep], sig[keep], sgd[keep])
    assert not stk.any()
    for k, s in enumerate(keep):
        assert ll[s] == llk[k]
        for a, b in zip(gps[s].factor(), gk[k].factor()):
            assert np.array_equal(np.tril(a) if a.ndim == 2 else a, np.tril(b) if b.ndim == 2 else b)
        for a, b in zip(gps[s].predict(Xs), gk[k].predict(Xs)):
            assert np.array_equal(a, b)
    for s in (1, 3):
        with pytest.raises(api.BossError) as e:
            gps[s].predict(Xs)
        assert e.value.code == api.BOSS_E_NOT_FITTED
    close_all(gps), close_all(gk)
    # the nonstationary model: a negative lengthscale, and a duplicated point under zero noise
    d, N, S, M = 2, 200, 5, 33
    X, y, lam, amp, noi, Xs, lam_s, amp_s = ns_case(d, N, S, M, seed=2)
    X[:, 1] = X[:, 0]
    lam[:, 1, :] = lam[:, 0, :]
    amp[1, :] = amp[0, :]
    lam2, noi2 = lam.copy(order="F"), noi.copy(order="F")
    lam2[0, 5, 1] = -0.5
    noi2[:, 3] = 0.0
    gps, ll, st = api.ngp_fit_batch(X, y, lam2, amp, noi2)
    assert st.tolist() == [0, api.BOSS_E_INVALID, 0, api.BOSS_E_NOT_PD, 0] and ll[1] == -np.inf and ll[3] == -np.inf
    gk, llk, stk = api.ngp_fit_batch(X, y, lam[:, :, keep], amp[:, keep], noi[:, keep])
    assert not stk.any()
    for k, s in enumerate(keep):
        assert ll[s] == llk[k]
        for a, b in zip(gps[s].factor(), gk[k].factor()):
            assert np.array_equal(np.tril(a) if a.ndim == 2 else a, np.tril(b) if b.ndim == 2 else b)
        for a, b in zip(gps[s].predict(Xs, lam_s[:, :, s], amp_s[:, s]), gk[k].predict(Xs, lam_s[:, :, s], amp_s[:, s])):
            assert np.array_equal(a, b)
    for s in (1, 3):
        with pytest.raises(api.BossError) as e:
            gps[s].predict(Xs, lam_s[:, :, s], amp_s[:, s])
        assert e.value.code == api.BOSS_E_NOT_FITTED
    with pytest.raises(api.BossError) as e:                       # the set call refuses an unfitted member as well
        api.ngp_predict_set(gps, Xs, lam_s, amp_s)
    assert e.value.code == api.BOSS_E_NOT_FITTED
    close_all(gps), close_all(gk)


def test_released_storage_is_reused_without_leaking_into_the_next_set(api, O):
    """The slab of a set whose last member is gone stays with the context for the next fit — of either model: a larger set, a smaller
    one in the block it left behind, a larger one again, with a member kept alive across the hand-over; every posterior agrees with
    the oracle, i.e. nothing of the previous tenant's factors, inverses or parameters is read."""
    import ctypes as C
    lib = api.load_library()
    lib.boss_debug_slab_cache_bytes.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    keep = None
    Xs_g = np.random.default_rng(3).uniform(0, 1, (3, 40))
    for rnd, (model, a, b, S) in enumerate([("ggp", 150, 3, 5), ("ngp", 300, 3, 3), ("ggp", 40, 3, 4), ("ngp", 700, 3, 6), ("ggp", 150, 3, 5)]):
        if model == "ggp":
            X, y, dY, lam, amp, sig, sgd = grad_case(a, b, S, seed=50 + rnd)
            gps, ll, st = api.ggp_fit_batch(X, y, dY, "matern52", lam, amp, sig, sgd)
            posts = [O.gradient_gp_fit(X, y, dY, "matern52", lam[:, s], amp[s], sig[s], sgd[s]) for s in range(S)]
            pred = [(lambda g=g: g.predict(Xs_g)) for g in gps]
            want = [O.gradient_gp_mean_and_var(p, Xs_g) for p in posts]
            a2 = amp ** 2
        else:
            X, y, lam, amp, noi, Xs, lam_s, amp_s = ns_case(b, a, S, 40, seed=50 + rnd)
            gps, ll, st = api.ngp_fit_batch(X, y, lam, amp, noi)
            posts = [O.nonstationary_fit(X, y, lam[:, :, s], amp[:, s], noi[:, s]) for s in range(S)]
            pred = [(lambda g=g, s=s: g.predict(Xs, lam_s[:, :, s], amp_s[:, s])) for s, g in enumerate(gps)]
            want = [O.nonstationary_mean_and_var(p, Xs, lam_s[:, :, s], amp_s[:, s]) for s, p in enumerate(posts)]
            a2 = (amp_s ** 2).max(0)
        assert not st.any()
        for s in range(S):
            assert abs(ll[s] - posts[s].logpdf) <= 1e-9 * (1 + abs(posts[s].logpdf)), (rnd, s)
            mu, var = pred[s]()
            assert np.allclose(mu, want[s][0], rtol=0, atol=1e-9 * (1 + np.abs(want[s][0]).max())), (rnd, s)
            assert np.allclose(var, want[s][1], rtol=0, atol=1e-9 * a2[s] + 1e-12), (rnd, s)
        if keep is not None:                                      # the survivor of the previous round still describes ITS data
            g_old, f_old, w_old, a_old = keep
            mu, var = f_old()
            assert np.allclose(mu, w_old[0], rtol=0, atol=1e-9 * (1 + np.abs(w_old[0]).max())) and np.allclose(var, w_old[1], rtol=0, atol=1e-9 * a_old + 1e-12), rnd
            g_old.close()
            nbytes = C.c_size_t(0)
            lib.boss_debug_slab_cache_bytes(0, C.byref(nbytes))
            if not os.environ.get("BOSS_POISON_ALLOC") and os.environ.get("BOSS_SLAB_CACHE") != "0":
                assert nbytes.value > 0, "the released slab was not parked for the next fit"
        keep = (gps[0], pred[0], want[0], a2[0])
        for g in gps[1:]:
            g.close()
    keep[0].close()
