"""Warps on the device: the two stage kernels against their host twins (pinned to 50 digits by tests/test_warp_host.py), the one-call
paths against the staged composition of existing calls (bit for bit), against the 50-digit truths of tests/golden/warp.json, and a
device-warped HipTransformedModel under both maximizers against the plain-closure host path of the same model.

Device against host twin: the project's interpreter bars, values 1e-12·max(1, max|·|), gradients 1e-11·max(1, max|·|)."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _chain8(z):
    """A joint transform of P = 8 outputs: each output mixes in its predecessor."""
    y, s = z[:8], z[8:]
    m = [y[0]] + [y[i] + 0.1 * y[i - 1] for i in range(1, 8)]
    sd = [s[0]] + [np.sqrt(s[i] ** 2 + (0.1 * s[i - 1]) ** 2) for i in range(1, 8)]
    return m + sd


@pytest.fixture(scope="module")
def stage_cfgs(B):
    """name -> (warp, d_user, d_model, P, nI_in, nI_out, lo, hi): (d_user, d_model) in {(1,1), (2,3), (3,2), (16,16)}, P in {1, 2, 8}; the
    last one's programs are hand-built with 64 instructions per output."""
    api = B.api
    nI = lambda prog: max(q.code.shape[0] for q in prog.outputs)      # noqa: E731

    def make(ip, P, op, lo, hi):
        return (api.WarpProgram(ip, P, op), ip.d, ip.P, P, nI(ip), nI(op), lo, hi)
    P2 = lambda z: (lambda m, s: list(m) + list(s))(*W.out_mix(z[:2], z[2:], np))      # noqa: E731
    return {
        "1to1-P1": make(B.trace_mean(lambda x: [np.log(x[0] + 2.0)], 1, 0, 1), 1,
                        B.trace_mean(lambda z: [np.log(z[0]), z[1] / z[0]], 2, 0, 2), 0.2, 1.2),
        "2to3-P2": make(B.trace_mean(W.in_closure("feature-log"), 2, 0, 3), 2, B.trace_mean(P2, 4, 0, 4), 0.2, 1.2),
        "3to2-P8": make(B.trace_mean(W.in_closure("kuma-mix"), 3, 0, 2), 8, B.trace_mean(_chain8, 16, 0, 16), 0.2, 1.2),
        "16to16-P8-64instr": make(W.big_program(api, 16, 16), 8, W.big_program(api, 16, 16), 0.2, 1.2),
    }


def _moments(rng, S, P, M, dm):
    return (rng.uniform(1.0, 2.0, (S, P, M)), rng.uniform(0.05, 0.4, (S, P, M)), rng.standard_normal((S, P, dm, M)),
            rng.standard_normal((S, P, dm, M)))


def _bars(*pairs):
    """err/bar of (got, want, tol) triples, bar = tol·max(1, max|want|)."""
    return max(float(np.abs(g - w).max()) / (tol * max(1.0, float(np.abs(w).max()))) for g, w, tol in pairs)


def test_the_launch_rule_matches_its_restatement(stage_cfgs):
    seen = set()
    for name, (w, du, dm, P, ni, no, _, _) in stage_cfgs.items():
        for grad in (False, True):
            for n in (1, 63, 64, 65, 257):
                wx, lx = w.workgroup(0, n, grad)
                wm, lm = w.workgroup(1, n, grad, dm)
                sx, sm = W.slots_x(du, ni, grad), W.slots_m(P, no, dm, grad)
                assert (wx, lx) == (W.waves(sx, n), 512 * sx * W.waves(sx, n)), (name, grad, n)
                assert (wm, lm) == (W.waves(sm, n), 512 * sm * W.waves(sm, n)), (name, grad, n)
                seen |= {wx, wm}
    big = stage_cfgs["16to16-P8-64instr"][0]
    assert big.workgroup(0, 257, True) == (1, 80 * 1024) and big.workgroup(1, 257, True, 16) == (1, 88 * 1024)      # the longest cases: one wave, inside the LDS
    assert {1, 2, 4} <= seen and W.waves(40, 257) == 3       # (33 to 42 slots: three waves)


@pytest.mark.parametrize("name", ["1to1-P1", "2to3-P2", "3to2-P8", "16to16-P8-64instr"])
def test_stage_kernels_match_their_host_twins(stage_cfgs, name):
    w, du, dm, P, _, _, lo, hi = stage_cfgs[name]
    worst = 0.0
    for M in (1, 63, 64, 65, 257):
        rng = np.random.default_rng(1000 + M)
        Xs = rng.uniform(lo, hi, (du, M))
        Xh, Jh = w.apply_host(Xs, True)
        Xd, Jd = w.apply(Xs, True)
        worst = max(worst, _bars((Xd, Xh, 1e-12), (Jd, Jh, 1e-11)))
        assert np.array_equal(w.apply(Xs, True)[0], Xd) and np.array_equal(w.apply(Xs, True)[1], Jd)      # a second call: the same bits
        assert np.array_equal(w.apply(Xs, False)[0], Xd)
        for S in (1, 3):
            mu_, var_, dmu_, dvar_ = _moments(rng, S, P, M, dm)
            if M > 2:
                var_[S - 1, P - 1, 2] = -4e-9                # inside the clip
                var_[0, 0, 1] = 0.0
            h = w.moments_host(mu_, var_, dmu_, dvar_, Jh)
            d = w.moments(mu_, var_, dmu_, dvar_, Jh)
            worst = max(worst, _bars((d[0], h[0], 1e-12), (d[1], h[1], 1e-12), (d[2], h[2], 1e-11), (d[3], h[3], 1e-11)))
            again = w.moments(mu_, var_, dmu_, dvar_, Jh)
            assert all(np.array_equal(a, b) for a, b in zip(d, again))
            dv = w.moments(mu_, var_)                        # values alone: the same bits
            assert np.array_equal(dv[0], d[0]) and np.array_equal(dv[1], d[1])
    print(f"[warp-gpu] {name}: worst device-vs-host error {worst:.3e} of its bound")
    assert worst <= 1.0


def test_stage_conventions_on_the_device(B, stage_cfgs, api):
    """A variance below the clip under both conventions, a NaN candidate, and the identity output program, as on the host."""
    w, du, dm, P = stage_cfgs["2to3-P2"][:4]
    rng = np.random.default_rng(5)
    M = 70
    Xs = rng.uniform(0.2, 1.2, (du, M))
    _, J = w.apply(Xs, True)
    mu_, var_, dmu_, dvar_ = _moments(rng, 2, P, M, dm)
    clean = w.moments(mu_, var_, dmu_, dvar_, J)
    var_[1, 1, 66] = -1e-3
    with pytest.raises(api.DomainError) as e:
        w.moments(mu_, var_, dmu_, dvar_, J)
    assert e.value.bad_index == 66
    got = w.moments(mu_, var_, dmu_, dvar_, J, check=False)
    host = w.moments_host(mu_, var_, dmu_, dvar_, J, check=False)
    assert np.array_equal(got[1][1, :, 66], var_[1, :, 66]) and np.array_equal(got[0][1, :, 66], mu_[1, :, 66])
    assert np.all(got[2][1, :, :, 66] == 0.0) and np.all(got[3][1, :, :, 66] == 0.0) and np.all(host[2][1, :, :, 66] == 0.0)
    keep = np.ones((2, M), bool)
    keep[1, 66] = False
    for a, b in zip(got, clean):
        assert np.array_equal(np.moveaxis(a, -1, 1)[keep], np.moveaxis(b, -1, 1)[keep])      # the neighbours' bits
    Xb = Xs.copy()
    Xb[1, 64] = np.nan
    xb = w.apply(Xb, True)
    ok = np.arange(M) != 64
    ref = w.apply(Xs, True)
    assert np.isnan(xb[0][1, 64]) and np.array_equal(xb[0][:, ok], ref[0][:, ok]) and np.array_equal(xb[1][ok], ref[1][ok])
    wi = W.warp_program(B, "kuma-mix", with_out=False)      # identity output program: moments pass through, only J' is applied
    Ji = rng.uniform(-2.0, 2.0, (M, 2, 3))
    mu_, var_, dmu_, dvar_ = _moments(rng, 3, 2, M, 2)
    var_[2, 1, 5] = -3e-9
    got = wi.moments(mu_, var_, dmu_, dvar_, Ji)
    host = wi.moments_host(mu_, var_, dmu_, dvar_, Ji)
    assert np.array_equal(got[0], mu_) and np.array_equal(got[1], var_)
    assert _bars((got[2], host[2], 1e-11), (got[3], host[3], 1e-11)) <= 1.0


# ---------------------------------------------------------------------------------------------- staged composition
KERNEL = "matern52"


def _model_space(B, name, N, S, seed):
    """gps[s][p] fitted on model-space data of the case's warp (d_model inputs), the user-space training X and the constant prior mean."""
    du, dm, _, _, P, win = W.CASES[name][:6]
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.2, 1.2, (du, N))
    X_ = np.asfortranarray(np.array([np.asarray(win(X[:, j], np), float) for j in range(N)]).T)
    gps = []
    for s in range(S):
        row = []
        for p in range(P):
            y = W.PRIOR_MEAN + 0.4 * np.sin(2.0 * X_.sum(0) + p) + 0.02 * rng.standard_normal(N)
            g = B.api.GP(X_, y, KERNEL)
            g.update(np.full(dm, (0.5 + 0.1 * s) * np.sqrt(dm)), 0.6 + 0.1 * p, 0.05 + 0.01 * s, np.full(N, W.PRIOR_MEAN))
            row.append(g)
        gps.append(row)
    return gps


def _close(gps):
    for row in gps:
        for g in row:
            g.close()


@pytest.mark.parametrize("N", [40, 136])
@pytest.mark.parametrize("M", [6, 65])
def test_input_warp_alone_equals_the_plain_calls_on_warped_candidates(B, api, N, M):
    name = "feature-log"
    P = W.CASES[name][4]
    w = W.warp_program(B, name, with_out=False)
    Xs = np.random.default_rng(N + M).uniform(0.25, 1.15, (2, M))
    X_ = w.apply(Xs)[0]
    mask = np.ones(M, bool)
    mask[M // 2] = False
    for S in (1, 3):
        gps = _model_space(B, name, N, S, 7)
        try:
            means = np.full((S, P, M), W.PRIOR_MEAN)
            cand = api.Candidates(X_)
            want = api.acq_ei(gps, cand, [1.0], [2.6], 2.2, mask, means)
            cand.close()
            got = w.acq_ei(gps, Xs, [1.0], [2.6], 2.2, mask, means)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
            assert w.acq_ei(gps, Xs, [1.0], [2.6], 2.2, mask, means, want_acq=False)[1:] == want[1:]
            mu, var = w.predict(gps, Xs, means)
            for s in range(S):
                for p in range(P):
                    m1, v1 = gps[s][p].predict(X_, means[s, p])
                    assert np.array_equal(mu[s, p], m1) and np.array_equal(var[s, p], v1)
        finally:
            _close(gps)


def _staged(api, w, gps, Xs, means):
    """boss_warp_apply -> boss_gp_predict_grad per output -> boss_warp_moments, sample by sample: [S] of (mu, var, dmu, dvar)."""
    X_, J = w.apply(Xs, True)
    out = []
    for s, row in enumerate(gps):
        r = [g.predict_grad(X_, means[s, p], None) for p, g in enumerate(row)]
        out.append(w.moments(*(np.stack([q[k] for q in r]) for k in range(4)), J))
    return out


@pytest.mark.parametrize("N", [40, 136])
@pytest.mark.parametrize("M", [6, 65])
def test_one_call_equals_the_staged_composition(B, api, N, M):
    name = "kuma-mix"
    P = W.CASES[name][4]
    w = W.warp_program(B, name)
    Xs = np.random.default_rng(N * M).uniform(0.25, 1.15, (3, M))
    coefs, ymax, best = [1.0, 0.3], [2.6, np.inf], 2.3
    mask = np.ones(M, bool)
    mask[1] = False
    for S in (1, 3):
        gps = _model_space(B, name, N, S, 9)
        try:
            means = np.full((S, P, M), W.PRIOR_MEAN)
            st = _staged(api, w, gps, Xs, means)
            mu, var, dmu, dvar = w.predict_grad(gps, Xs, means)
            acq, dacq = w.acq_ei_grad(gps, Xs, coefs, ymax, best, mask, means)
            a_st = [api.acq_ei_grad_moments(*q, coefs, ymax, best, mask) for q in st]
            mu_v, var_v = w.predict(gps, Xs, means)
            acq_v, am, mx = w.acq_ei(gps, Xs, coefs, ymax, best, mask, means)
            if S == 1:
                for got, want in zip((mu[0], var[0], dmu[0], dvar[0], acq, dacq), st[0] + a_st[0]):
                    assert np.array_equal(got, want)
                # the value calls against their own staged chain: boss_gp_predict -> boss_warp_moments -> boss_acq_ei_moments
                X_ = w.apply(Xs)[0]
                pv = [g.predict(X_, means[0, p]) for p, g in enumerate(gps[0])]
                sv = w.moments(np.stack([q[0] for q in pv]), np.stack([q[1] for q in pv]))
                assert np.array_equal(mu_v[0], sv[0]) and np.array_equal(var_v[0], sv[1])
                want = api.acq_ei_moments(sv[0][None], sv[1][None], coefs, ymax, best, mask)
                assert np.array_equal(acq_v, want[0]) and (am, mx) == (want[1], want[2])
            else:
                ref = [np.stack([q[k] for q in st]) for k in range(4)]
                r = _bars((mu, ref[0], 1e-12), (var, ref[1], 1e-12), (dmu, ref[2], 1e-11), (dvar, ref[3], 1e-11),
                          (acq, np.mean([a for a, _ in a_st], axis=0), 1e-12), (dacq, np.mean([g for _, g in a_st], axis=0), 1e-11),
                          (mu_v, ref[0], 1e-12), (var_v, ref[1], 1e-12), (acq_v, np.mean([a for a, _ in a_st], axis=0), 1e-12))
                print(f"[warp-gpu] N {N} M {M} S 3: one call vs staged chain {r:.3e} of the bound")
                assert r <= 1.0 and am == int(np.argmax(acq_v)) and mx == acq_v[am]
            assert acq[1] == 0.0 and np.all(dacq[:, 1] == 0.0)      # the mask
            again = w.acq_ei_grad(gps, Xs, coefs, ymax, best, mask, means)
            assert np.array_equal(again[0], acq) and np.array_equal(again[1], dacq)
        finally:
            _close(gps)


def test_one_call_refusals_on_the_device(B, api):
    w = W.warp_program(B, "kuma-mix")
    gps = _model_space(B, "kuma-mix", 40, 1, 3)
    rng = np.random.default_rng(0)
    Xg = np.asfortranarray(rng.uniform(0, 1, (2, 20)))
    ns = api.GibbsGP(Xg, np.sin(Xg.sum(0)))
    other = api.GP(np.asfortranarray(rng.uniform(0, 1, (3, 20))), rng.standard_normal(20), KERNEL)
    other.update(np.full(3, 0.5), 1.0, 0.1, None)
    try:
        Xs = rng.uniform(0.25, 1.15, (3, 6))
        with pytest.raises(api.BossError, match="nonstationary"):
            w.predict([[gps[0][0], ns]], Xs)
        with pytest.raises(api.BossError, match="x_dim"):
            w.predict([[gps[0][0], other]], Xs)
        with pytest.raises(api.BossError, match="created for 2 outputs"):
            w.predict([[gps[0][0]]], Xs)
        mu, var = w.predict(gps, Xs, np.full((1, 2, 6), W.PRIOR_MEAN))      # every handle is still usable
        assert np.all(np.isfinite(mu)) and np.all(var >= 0)
    finally:
        _close(gps)
        ns.close()
        other.close()


# ---------------------------------------------------------------------------------------------- truths
@pytest.mark.parametrize("name", list(W.CASES))
def test_one_call_predict_grad_against_50_digit_truths(B, api, name):
    c = W.load()["cases"][name]
    du, dm, N, M, P, _, _, kernel, _ = W.CASES[name]
    _, Xs, X_, Y_ = W.data(name)
    lam, amp, sig = W.hyper(name)
    gps = [[api.GP(X_, Y_[p], kernel) for p in range(P)]]
    try:
        for p, g in enumerate(gps[0]):
            g.update(lam, amp[p], sig[p], np.full(N, W.PRIOR_MEAN))
        w = W.warp_program(B, name)
        means = np.full((1, P, M), W.PRIOR_MEAN)
        mu, var, dmu, dvar = w.predict_grad(gps, Xs, means)
        vb, gb = W.chain_bars(c, N)
        ev = max(np.abs(mu[0] - c["mu"]).max(), np.abs(var[0] - c["var"]).max())
        eg = max(np.abs(dmu[0] - c["dmu"]).max(), np.abs(dvar[0] - c["dvar"]).max())
        print(f"[warp-gpu] {name}: value err/bar {ev / vb:.3e}, gradient err/bar {eg / gb:.3e} (cond {max(c['cond']):.3g}, L {c['L']:.3g})")
        assert ev <= vb and eg <= gb
        mv = w.predict(gps, Xs, means)
        assert max(np.abs(mv[0][0] - c["mu"]).max(), np.abs(mv[1][0] - c["var"]).max()) <= vb
    finally:
        _close(gps)


# ---------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def problems(B):
    """The same transformed model twice — traced transforms (device) and plain closures (host) — over N = 40 points, P = 2."""
    fw, bw = W.sliced_closures("logw-affine")
    win = W.in_closure("logw-affine")
    rng = np.random.default_rng(21)
    X = rng.uniform(0.2, 1.2, (2, 40))
    X_ = np.array([win(X[:, j]) for j in range(40)]).T
    Y_ = np.stack([W.PRIOR_MEAN + 0.4 * np.sin(2.0 * X_.sum(0) + p) + 0.02 * rng.standard_normal(40) for p in range(2)])
    Y = np.stack([a * Y_[i] + b for i, (a, b) in enumerate(W.AFFINE)])          # user space
    data = B.ExperimentData(np.asfortranarray(X), Y)
    dom = B.Domain(bounds=([0.2, 0.2], [1.2, 1.2]))
    params = B.HipGPParams(np.full((2, 2), 0.7), [0.6, 0.7], [0.05, 0.06])

    def base():
        return B.HipGaussianProcess([B.MvLogNormal([0.0, 0.0], [1.0, 1.0])] * 2, [B.LogNormal(0.0, 1.0)] * 2, [B.LogNormal(-2.0, 1.0)] * 2,
                                    mean=[W.PRIOR_MEAN, W.PRIOR_MEAN], kernel=KERNEL)
    dev = B.HipTransformedModel(base(), B.DeviceInputTransform(win, 2, 2), B.DeviceSlicedOutputTransform(fw, bw))
    host = B.HipTransformedModel(base(), B.InputTransform(win), B.SlicedOutputTransform(fw, bw))
    mk = lambda m: B.BossProblem(f=None, model=m, data=data, domain=dom, acquisition=B.ExpectedImprovement(B.LinFitness([1.0, -0.2])),      # noqa: E731
                                 y_max=[np.inf, 0.0], params=params)
    return mk(dev), mk(host)


def test_device_warped_model_agrees_with_the_plain_closure_host_path(B, problems):
    pd, ph = problems
    assert pd.model.warp is not None and ph.model.warp is None
    pts = np.asfortranarray(np.random.default_rng(22).uniform(0.2, 1.2, (2, 64)))
    post_d, post_h = pd.model.model_posterior(pd.params, pd.data), ph.model.model_posterior(ph.params, ph.data)
    try:
        (md, vd), (mh, vh) = post_d.mean_and_var(pts), post_h.mean_and_var(pts)
        r = _bars((md, mh, 1e-12), (vd, vh, 1e-12))
        print(f"[warp-gpu] model: device-warped vs plain-closure mean_and_var {r:.3e} of the bound")
        assert r <= 1.0
        m1, v1 = post_d.mean_and_var(pts[:, 5])
        assert np.array_equal(m1, md[:, 5]) or _bars((m1, md[:, 5], 1e-12)) <= 1.0
        g = post_d.mean_and_var_grad(pts)
        assert _bars((g[0], md, 1e-12), (g[1], vd, 1e-12)) <= 1.0 and g[2].shape == (2, 2, 64) and g[3].shape == (2, 2, 64)
    finally:
        post_d.close()
        post_h.close()
    xd, vd_ = B.HipBatchAM(points=pts).maximize_acquisition(pd)
    xh, vh_ = B.HipBatchAM(points=pts).maximize_acquisition(ph)
    assert np.array_equal(xd, xh) and abs(vd_ - vh_) <= 1e-12 * max(1.0, abs(vh_)) and vd_ > 0.0
    # with both transforms None the model is its base model, bit for bit
    ident = B.HipTransformedModel(pd.model.base_model)
    tdata = pd.model.transform_data(pd.data)
    pi = B.BossProblem(f=None, model=ident, data=tdata, domain=pd.domain, acquisition=pd.acquisition, y_max=pd.y_max, params=pd.params)
    pb = B.BossProblem(f=None, model=pd.model.base_model, data=tdata, domain=pd.domain, acquisition=pd.acquisition, y_max=pd.y_max, params=pd.params)
    ri, rb = B.HipBatchAM(points=pts).maximize_acquisition(pi, return_all=True), B.HipBatchAM(points=pts, fused=False).maximize_acquisition(pb, return_all=True)
    assert np.array_equal(ri[1], rb[1])
    assert ident.data_loglike(tdata)(pd.params) == pd.model.base_model.data_loglike(tdata)(pd.params)
    assert pd.model.data_loglike(pd.data)(pd.params) == ident.data_loglike(tdata)(pd.params)       # the likelihood is the base model's on the transformed data


def test_gradient_ascent_climbs_and_its_gradients_are_the_staged_compositions(B, api, problems):
    pd, ph = problems
    am = B.HipGradientAM(x_prior=lambda r: r.uniform(0.2, 1.2, 2), multistart=8, iters=3, seed=3)
    posts = [pd.model.model_posterior(pd.params, pd.data)]
    log = []
    inner = am._value_and_grad
    am._value_and_grad = lambda prob, ps, X: (lambda r: (log.append((X.copy(), r[0].copy(), r[1].copy())), r)[1])(inner(prob, ps, X))
    try:
        x, v = am.maximize_acquisition(pd, posts=posts)
        assert len(log) == 4 and log[0][0].shape == (2, 8)
        assert v >= log[0][1].max() and np.all(x >= 0.2) and np.all(x <= 1.2)
        w = pd.model.warp
        gps = [[s.gp for s in posts[0].base.slices]]
        from boss_jl_amd.problem import best_so_far
        b = best_so_far(pd.acquisition.fitness, pd.data.Y, pd.y_max)
        for X, f, g in log:                                  # every iterate: value and gradient of the staged composition, bit for bit
            means = np.full((1, 2, X.shape[1]), W.PRIOR_MEAN)
            st = _staged(api, w, gps, X, means)[0]
            fa, ga = api.acq_ei_grad_moments(*st, pd.acquisition.fitness.coefs, pd.y_max, b, np.ones(X.shape[1], bool))
            assert np.array_equal(f, fa) and np.array_equal(g, ga)
        with pytest.raises(NotImplementedError, match="plain closure has no derivative"):
            B.HipGradientAM(x_prior=lambda r: r.uniform(0.2, 1.2, 2), multistart=2, iters=1, seed=3).maximize_acquisition(ph)
    finally:
        posts[0].close()


def test_fitters_fit_the_base_model_on_the_transformed_data(B, problems):
    pd, _ = problems
    import copy
    base_prob = copy.copy(pd)
    base_prob.model, base_prob.data = pd.model.base_model, pd.model.transform_data(pd.data)
    for fitter in (B.HipBatchedMAP(16, seed=1), B.HipGradientMAP(multistart=2, iters=2, seed=1), B.HipSampleOptMAP(samples=8, multistart=2, iters=2, seed=1)):
        a, b = fitter.estimate_parameters(pd), fitter.estimate_parameters(base_prob)
        assert a.loglike == b.loglike and np.array_equal(a.params.lengthscales, b.params.lengthscales)


def test_a_device_mean_under_the_warp_contributes_its_gradient(B, problems):
    """The base model's prior mean as a DeviceMean: m(x_) and ∂m/∂x_ at the warped points enter the one-call paths; the user-space
    gradients agree with central differences of the user-space moments (h = 1e-6: truncation ~1e-12·|f'''|, rounding ~1e-10·|f|)."""
    pd, _ = problems
    fw, bw = W.sliced_closures("logw-affine")
    base = B.HipGaussianProcess([B.MvLogNormal([0.0, 0.0], [1.0, 1.0])] * 2, [B.LogNormal(0.0, 1.0)] * 2, [B.LogNormal(-2.0, 1.0)] * 2,
                                mean=B.DeviceMean(lambda x: [2.0 + 0.3 * x[0], 2.0 - 0.2 * x[1] * x[0]], 2, 0, 2), kernel=KERNEL)
    model = B.HipTransformedModel(base, B.DeviceInputTransform(W.in_closure("logw-affine"), 2, 2), B.DeviceSlicedOutputTransform(fw, bw))
    post = model.model_posterior(pd.params, pd.data)
    try:
        X = np.asfortranarray(np.random.default_rng(31).uniform(0.3, 1.1, (2, 9)))
        mu, var, dmu, dvar = post.mean_and_var_grad(X)
        h = 1e-6
        for k in range(2):
            Xp, Xm = X.copy(), X.copy()
            Xp[k] += h
            Xm[k] -= h
            (mp_, vp), (mm, vm) = post.mean_and_var(Xp), post.mean_and_var(Xm)
            fd_m, fd_v = (mp_ - mm) / (2 * h), (vp - vm) / (2 * h)
            assert np.abs(fd_m - dmu[:, k, :]).max() <= 1e-6 * max(1.0, np.abs(dmu).max())
            assert np.abs(fd_v - dvar[:, k, :]).max() <= 1e-6 * max(1.0, np.abs(dvar).max())
        no_mean = B.HipTransformedModel(pd.model.base_model, model.input_transform, model.output_transform).model_posterior(pd.params, pd.data)
        assert np.abs(no_mean.mean_and_var(X)[0] - mu).max() > 1e-3          # the mean program is what differs
        no_mean.close()
    finally:
        post.close()


# ---------------------------------------------------------------------------------------------- gradient-observation handles
def _grad_model_space(B, name, n, S, seed):
    """gps[s][p]: gradient-observation handles (boss_ggp_*) fitted on model-space points, values and gradients of the case's warp."""
    du, dm, _, _, P, win = W.CASES[name][:6]
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.2, 1.2, (du, n))
    X_ = np.asfortranarray(np.array([np.asarray(win(X[:, j], np), float) for j in range(n)]).T)
    gps = []
    for s in range(S):
        row = []
        for p in range(P):
            y = W.PRIOR_MEAN + 0.4 * np.sin(2.0 * X_.sum(0) + p)
            dY = np.asfortranarray(np.repeat((0.8 * np.cos(2.0 * X_.sum(0) + p))[None, :], dm, axis=0))
            g = B.api.GradGP(X_, y, dY, KERNEL)
            g.update(np.full(dm, (0.5 + 0.1 * s) * np.sqrt(dm)), 0.6 + 0.1 * p, 0.05 + 0.01 * s, 0.1)
            row.append(g)
        gps.append(row)
    return gps


def _staged_nomean(w, gps, Xs):
    X_, J = w.apply(Xs, True)
    out = []
    for row in gps:
        r = [g.predict_grad(X_, None, None) for g in row]
        out.append(w.moments(*(np.stack([q[k] for q in r]) for k in range(4)), J))
    return out


@pytest.mark.parametrize("n", [12, 45])
@pytest.mark.parametrize("M", [6, 65])
def test_one_call_equals_the_staged_composition_on_gradient_observation_handles(B, api, n, M):
    """The same comparison as above on boss_ggp_* handles, n(1 + d_model) rows: the model's own accumulation kernels under the warp,
    d_model = 2 against d_user = 3, J' applied to their gradients.  S = 1 bit for bit, S = 3 within the interpreter bars."""
    name = "kuma-mix"
    w = W.warp_program(B, name)
    Xs = np.random.default_rng(n * M + 1).uniform(0.25, 1.15, (3, M))
    coefs, ymax, best = [1.0, 0.3], [2.6, np.inf], 2.3
    mask = np.ones(M, bool)
    mask[2] = False
    for S in (1, 3):
        gps = _grad_model_space(B, name, n, S, 13)
        try:
            st = _staged_nomean(w, gps, Xs)
            mu, var, dmu, dvar = w.predict_grad(gps, Xs)
            acq, dacq = w.acq_ei_grad(gps, Xs, coefs, ymax, best, mask)
            a_st = [api.acq_ei_grad_moments(*q, coefs, ymax, best, mask) for q in st]
            mu_v, var_v = w.predict(gps, Xs)
            acq_v, am, mx = w.acq_ei(gps, Xs, coefs, ymax, best, mask)
            assert np.all(np.isfinite(dacq)) and np.abs(dmu).max() > 0 and dacq.shape == (3, M)
            if S == 1:
                for got, want in zip((mu[0], var[0], dmu[0], dvar[0], acq, dacq), st[0] + a_st[0]):
                    assert np.array_equal(got, want)
                X_ = w.apply(Xs)[0]
                pv = [g.predict(X_) for g in gps[0]]
                sv = w.moments(np.stack([q[0] for q in pv]), np.stack([q[1] for q in pv]))
                assert np.array_equal(mu_v[0], sv[0]) and np.array_equal(var_v[0], sv[1])
                want = api.acq_ei_moments(sv[0][None], sv[1][None], coefs, ymax, best, mask)
                assert np.array_equal(acq_v, want[0]) and (am, mx) == (want[1], want[2])
            else:
                ref = [np.stack([q[k] for q in st]) for k in range(4)]
                am_ = np.mean([a for a, _ in a_st], axis=0)
                r = _bars((mu, ref[0], 1e-12), (var, ref[1], 1e-12), (dmu, ref[2], 1e-11), (dvar, ref[3], 1e-11), (acq, am_, 1e-12),
                          (dacq, np.mean([g for _, g in a_st], axis=0), 1e-11), (mu_v, ref[0], 1e-12), (var_v, ref[1], 1e-12), (acq_v, am_, 1e-12))
                print(f"[warp-gpu] gradient observations n {n} M {M} S 3: one call vs staged chain {r:.3e} of the bound")
                assert r <= 1.0
            with pytest.raises(api.BossError, match="no prior mean"):      # these posteriors take none, under a warp as without
                w.predict(gps, Xs, np.zeros((S, 2, M)))
        finally:
            _close(gps)


def test_transformed_gradient_model_end_to_end(B):
    """HipTransformedModel over a HipGradientGaussianProcess: user-space GradientData, posterior, both maximizers, the fitter."""
    fw, bw = W.sliced_closures("logw-affine")
    win = W.in_closure("logw-affine")
    rng = np.random.default_rng(41)
    X = np.asfortranarray(rng.uniform(0.2, 1.2, (2, 14)))
    X_ = np.array([win(X[:, j]) for j in range(14)]).T
    J = [np.array([[1 / (x[0] + 0.1), 0.0], [0.5 / (x[1] + 0.5 * x[0] + 0.1), 1 / (x[1] + 0.5 * x[0] + 0.1)]]) for x in X.T]
    Y_ = np.stack([np.sin(2.0 * X_.sum(0) + p) for p in range(2)])
    dY_ = np.stack([np.repeat((2.0 * np.cos(2.0 * X_.sum(0) + p))[None, :], 2, axis=0) for p in range(2)])       # [P, d, n]
    Y = np.stack([a * Y_[i] + b for i, (a, b) in enumerate(W.AFFINE)])
    dY = np.stack([np.diag([a for a, _ in W.AFFINE]) @ dY_[:, :, j] @ J[j] for j in range(14)], axis=2)
    data = B.GradientData(X, Y, dY)
    pri = [B.LogNormal(0.0, 1.0)] * 2
    base = B.HipGradientGaussianProcess([B.MvLogNormal([0.0, 0.0], [1.0, 1.0])] * 2, pri, [B.LogNormal(-2.0, 1.0)] * 2, [B.LogNormal(-2.0, 1.0)] * 2,
                                        kernel=KERNEL)
    model = B.HipTransformedModel(base, B.DeviceInputTransform(win, 2, 2), B.DeviceSlicedOutputTransform(fw, bw))
    params = B.HipGradientGPParams(np.full((2, 2), 0.7), [0.8, 0.9], [0.05, 0.06], [0.1, 0.1])
    prob = B.BossProblem(f=None, model=model, data=data, domain=B.Domain(bounds=([0.2, 0.2], [1.2, 1.2])),
                         acquisition=B.ExpectedImprovement(B.LinFitness([1.0, -0.2])), y_max=[np.inf, 3.0], params=params)
    td = model.transform_data(data)
    assert np.abs(td.dY - dY_).max() <= 1e-12 and np.abs(td.Y - Y_).max() <= 1e-14
    post = model.model_posterior(params, data)
    direct = base.model_posterior(params, td)
    try:
        # at the training points the posterior mean returns to the user-space observations (noise 0.05: to a few per cent)
        mu_tr, _ = post.mean_and_var(X)
        assert np.abs(mu_tr - Y).max() < 0.2
        Xc = np.asfortranarray(rng.uniform(0.3, 1.1, (2, 9)))
        mu, var, dmu, dvar = post.mean_and_var_grad(Xc)
        m_, v_ = direct.mean_and_var(np.array([win(Xc[:, j]) for j in range(9)]).T)      # the base posterior at the warped points, then the affine map
        want_mu = np.stack([a * m_[i] + b for i, (a, b) in enumerate(W.AFFINE)])
        assert _bars((mu, want_mu, 1e-12), (var, np.stack([a * a * v_[i] for i, (a, _) in enumerate(W.AFFINE)]), 1e-12)) <= 1.0
        h = 1e-6
        for k in range(2):
            Xp, Xm = Xc.copy(), Xc.copy()
            Xp[k] += h
            Xm[k] -= h
            (mp_, vp), (mm, vm) = post.mean_and_var(Xp), post.mean_and_var(Xm)
            assert np.abs((mp_ - mm) / (2 * h) - dmu[:, k, :]).max() <= 1e-6 * max(1.0, np.abs(dmu).max())
            assert np.abs((vp - vm) / (2 * h) - dvar[:, k, :]).max() <= 1e-6 * max(1.0, np.abs(dvar).max())
        pts = np.asfortranarray(rng.uniform(0.2, 1.2, (2, 64)))
        Xall, acq = B.HipBatchAM(points=pts).maximize_acquisition(prob, return_all=True, posts=[post])
        xb, vb = B.HipBatchAM(points=pts).maximize_acquisition(prob, posts=[post])
        assert np.array_equal(xb, pts[:, int(np.argmax(acq))]) and vb == acq.max() and np.all(np.isfinite(acq))
        xg, vg = B.HipGradientAM(x_prior=lambda r: r.uniform(0.2, 1.2, 2), multistart=8, iters=3, seed=5).maximize_acquisition(prob, posts=[post])
        assert np.isfinite(vg) and np.all(xg >= 0.2) and np.all(xg <= 1.2)
    finally:
        post.close()
        direct.close()
    import copy
    base_prob = copy.copy(prob)
    base_prob.model, base_prob.data = base, td
    fitter = B.HipGradientMAP(multistart=2, iters=2, seed=1)
    a, b = fitter.estimate_parameters(prob), fitter.estimate_parameters(base_prob)
    assert a.loglike == b.loglike and np.array_equal(a.params.grad_noise_std, b.params.grad_noise_std)
    assert model.data_loglike(data)(params) == base.data_loglike(td)(params)
