"""Mean programs on the device (boss_mean_eval) and everything a DeviceMean is wired into.

Device against the host interpreter (boss_mean_eval_host, pinned to 50 digits by tests/test_mean_program_host.py) with the bounds the
project holds this interpreter to on the device (tests/test_gpu_fitness_mc.py): values 1e-12·max(1, max|m|), Jacobians
1e-11·max(1, max|∇|).  Plumbing is checked bit for bit: a model call over a DeviceMean must equal the api call fed the arrays that
boss_mean_eval returned — layout, set order and the output loop, with no conditioning-dependent tolerance."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mean_program_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["M1", "M2", "M3", "M4", "M5", "M6", "S16", "T1", "W3"]


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
def means(B):
    out = {name: B.DeviceMean(*spec) for name, spec in cases.M.items()}
    out["M6"] = cases.HandMean(cases.big_mean_program(B.api))
    return out


def _bounds(mh, jth, jxh):
    vb = 1e-12 * max(1.0, np.abs(mh).max())
    gmax = max([np.abs(a).max() for a in (jth, jxh) if a is not None and a.size] + [0.0])
    return vb, 1e-11 * max(1.0, gmax)


def test_the_cases_cover_the_shapes_and_both_workgroup_shapes(means):
    """P in {1, 2, 16}, T in {0, 1, 5}, d in {1, 6, 16}; M6 runs as one wave per workgroup, the three-instruction program as four —
    from the library's own launch rule (boss_debug_mean_block) and its restatement in the cases module."""
    progs = {k: v.program for k, v in means.items()}
    assert {1, 2, 16} <= {p.P for p in progs.values()}
    assert {0, 1, 5} <= {p.T for p in progs.values()}
    assert {1, 6, 16} <= {p.d for p in progs.values()}
    seen = set()
    for name, p in progs.items():
        nI = max(q.code.shape[0] for q in p.outputs)
        for grad in (False, True):
            for n in (1, 63, 64, 65, 257):
                waves, lds = p.workgroup(n, grad)
                assert waves == cases.mean_waves(p.d + p.T, nI, grad, n), (name, grad, n)
                assert lds == 512 * max(1, cases.mean_slots(p.d + p.T, nI, grad)) * waves and lds <= 96 * 1024
                seen.add(waves)
    assert progs["M6"].workgroup(257, True) == (1, 96 * 1024)
    assert progs["T1"].outputs[0].code.shape[0] == 3 and progs["T1"].workgroup(257, True)[0] == 4
    assert seen == {1, 2, 3, 4}


@pytest.mark.parametrize("name", NAMES)
def test_device_matches_the_host_interpreter(means, name):
    prog = means[name].program
    worst_v = worst_g = 0.0
    for n in (1, 63, 64, 65, 257):
        for S in (1, 3):
            X, Th = cases.points(100 + n + S, prog.d, prog.T, n, S)
            for layout in (0, 1):
                mh, jth, jxh = prog.eval_host(X, Th, layout, prog.T > 0, True)
                md, jtd, jxd = prog.eval_device(X, Th, layout, prog.T > 0, True)
                vb, gb = _bounds(mh, jth, jxh)
                ev = np.abs(md - mh).max()
                eg = max([np.abs(a - b).max() for a, b in ((jtd, jth), (jxd, jxh)) if a is not None and a.size] + [0.0])
                worst_v, worst_g = max(worst_v, ev / vb), max(worst_g, eg / gb)
                assert md.shape == mh.shape and ev <= vb, (name, n, S, layout, ev, vb)
                assert eg <= gb, (name, n, S, layout, eg, gb)
                assert (jtd is None) == (prog.T == 0)
    print(f"[mean-gpu] {name}: worst value error {worst_v:.3e} of its bound, worst Jacobian error {worst_g:.3e} of its bound")
    # one Jacobian, the other, neither (the sweep is skipped): the same numbers; a second call: the same bits
    X, Th = cases.points(7, prog.d, prog.T, 65, 3)
    full = prog.eval_device(X, Th, 0, prog.T > 0, True)
    again = prog.eval_device(X, Th, 0, prog.T > 0, True)
    for a, b in zip(full, again):
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)
    only_x = prog.eval_device(X, Th, 0, False, True)
    none = prog.eval_device(X, Th, 0, False, False)
    assert only_x[1] is None and np.array_equal(only_x[2], full[2]) and np.array_equal(only_x[0], full[0])
    assert none[1] is None and none[2] is None and np.array_equal(none[0], full[0])
    if prog.T:
        only_t = prog.eval_device(X, Th, 0, True, False)
        assert only_t[2] is None and np.array_equal(only_t[1], full[1]) and np.array_equal(only_t[0], full[0])


def test_a_nan_point_leaves_its_neighbours_exact(B):
    dm = B.DeviceMean(lambda x, th: [np.log(x[0]) * th[0] + x[1], x[0] * th[0]], 2, 1, 2)
    rng = np.random.default_rng(2)
    X = rng.uniform(0.5, 2.0, (2, 130))
    Th = np.array([[0.7, -1.1]])
    clean = dm.program.eval_device(X, Th, 0, True, True)
    Xb = X.copy()
    Xb[0, [0, 64, 77, 129]] = -1.0                                # LOG of a negative number: NaN, as computed
    bad = dm.program.eval_device(Xb, Th, 0, True, True)
    hit = np.zeros(130, bool)
    hit[[0, 64, 77, 129]] = True
    assert np.all(np.isnan(bad[0][:, 0, hit])) and np.all(np.isfinite(bad[0][:, 1, hit]))
    host = dm.program.eval_host(Xb, Th, 0, True, True)
    assert np.array_equal(np.isnan(bad[0]), np.isnan(host[0])) and np.array_equal(np.isnan(bad[2]), np.isnan(host[2]))
    assert np.array_equal(bad[0][:, :, ~hit], clean[0][:, :, ~hit])
    assert np.array_equal(bad[1][:, :, ~hit, :], clean[1][:, :, ~hit, :]) and np.array_equal(bad[2][:, :, :, ~hit], clean[2][:, :, :, ~hit])


# ------------------------------------------------------------------------------------------ plumbing, bit for bit
def _pl(x, th):
    return np.array([th[0] + th[1] * x[0] + np.cos(th[2] * x[1]), 0.5 * th[0] - th[1] * x[1] + np.cos(th[2] * x[0])])


def _pl_jac(x, th):
    return np.array([[1.0, x[0], -x[1] * np.sin(th[2] * x[1])], [0.5, -x[1], -x[0] * np.sin(th[2] * x[0])]])


class Counted:
    """A closure that counts its calls."""

    def __init__(self, f):
        self.f, self.n = f, 0

    def __call__(self, *a):
        self.n += 1
        return self.f(*a)


def _priors(B, P, d):
    return dict(lengthscale_priors=[B.MvLogNormal([-0.5] * d, [0.3] * d)] * P, amplitude_priors=[B.LogNormal(-1.0, 0.3)] * P,
                noise_std_priors=[B.LogNormal(-2.5, 0.3)] * P)


@pytest.fixture(scope="module")
def plumbing(B):
    """N = 40, d = 2, P = 2, T = 3, S = 4: the DeviceMean model, the closure model (exact parametric_jac), data and parameter sets."""
    rng = np.random.default_rng(21)
    d, N, P = 2, 40, 2
    X = rng.uniform(0, 2, (d, N))
    truth = np.array([0.8, -0.6, 1.3])
    Y = np.stack([[_pl(X[:, j], truth)[i] for j in range(N)] for i in range(P)]) + 0.1 * np.sin(3 * X).sum(0) + 0.02 * rng.standard_normal((P, N))
    tp = [B.Normal(0.0, 2.0), B.Normal(0.0, 2.0), B.Normal(1.0, 1.0)]
    dm = B.DeviceMean(_pl, d, 3, P)
    dev = B.HipGaussianProcess(parametric=dm, theta_priors=tp, **_priors(B, P, d))
    host = B.HipGaussianProcess(parametric=_pl, parametric_jac=_pl_jac, theta_priors=tp, **_priors(B, P, d))
    sampler = dev.params_sampler()
    plist = [sampler(rng) for _ in range(4)]
    return dict(B=B, d=d, N=N, P=P, dm=dm, dev=dev, host=host, data=B.ExperimentData(X, Y), plist=plist,
                Xs=np.asfortranarray(rng.uniform(0.05, 1.95, (d, 100))))


def _problem(pl, model, params, y_max=(np.inf, 1.5)):
    B = pl["B"]
    return B.BossProblem(None, B.Domain((np.zeros(pl["d"]), 2 * np.ones(pl["d"]))), B.ExpectedImprovement(B.LinFitness([1.0, 0.3])), model,
                         pl["data"], y_max=list(y_max), params=params)


def _thetas(plist):
    return np.stack([p.theta for p in plist], axis=1)


def test_likelihood_calls_equal_the_api_fed_the_device_arrays(api, plumbing):
    pl = plumbing
    model, data, plist, P, d = pl["dev"], pl["data"], pl["plist"], pl["P"], pl["d"]
    m, jt, _ = pl["dm"].program.eval_device(data.X, _thetas(plist), api.MEAN_OUTPUT_MAJOR, True, False)      # P×S×N, P×S×N×T
    ll, grads = model.data_loglike_grad_batch(data, plist)
    tot, gth = np.zeros(4), np.zeros((4, 3))
    for i in range(P):
        lam = np.stack([p.lengthscales[:, i] for p in plist], axis=1)
        amp, sig = [p.amplitudes[i] for p in plist], [p.noise_std[i] for p in plist]
        l, st, gr, _, dth = api.loglike_grad_batch_mean(data.X, data.Y[i], model.kernel, lam, amp, sig, m[i], jt[i])
        assert np.all(st == 0)
        tot += l
        gth += dth.T
        for k in range(4):
            assert np.array_equal(grads[k].lengthscales[:, i], gr[:d, k]) and grads[k].amplitudes[i] == gr[d, k] and grads[k].noise_std[i] == gr[d + 1, k]
    assert np.array_equal(ll, tot) and all(np.array_equal(grads[k].theta, gth[k]) for k in range(4))
    tot2 = np.zeros(4)
    for i in range(P):
        lam = np.stack([p.lengthscales[:, i] for p in plist], axis=1)
        tot2 += api.loglike_batch(data.X, data.Y[i], model.kernel, lam, [p.amplitudes[i] for p in plist], [p.noise_std[i] for p in plist], m[i])[0]
    assert np.array_equal(model.data_loglike_batch(data, plist), tot2)
    # mean_values / mean_jacobians hand out the same blocks
    for i in range(P):
        assert np.array_equal(model.mean_values(data.X, plist[1], i), m[i, 1]) and np.array_equal(model.mean_jacobians(data.X, plist[1], i), jt[i, 1])


def test_bi_posterior_and_acquisition_equal_the_api_fed_the_device_arrays(api, plumbing):
    from boss_jl_amd.maximizer import acquisition_values
    from boss_jl_amd.problem import best_so_far, in_bounds, in_cons
    pl = plumbing
    model, data, plist, P, Xs = pl["dev"], pl["data"], pl["plist"], pl["P"], pl["Xs"]
    prob = _problem(pl, model, plist)
    posts = model.model_posterior(plist, data)
    acq, am, mx = acquisition_values(prob, posts, Xs)
    mX = pl["dm"].program.eval_device(data.X, _thetas(plist), api.MEAN_OUTPUT_MAJOR)[0]                     # P×S×N
    mXs = pl["dm"].program.eval_device(Xs, _thetas(plist), api.MEAN_SAMPLE_MAJOR)[0]                        # S×P×M
    rows = []
    for i in range(P):
        gps, _, st = api.fit_batch(data.X, data.Y[i], model.kernel, np.stack([p.lengthscales[:, i] for p in plist], axis=1),
                                   [p.amplitudes[i] for p in plist], [p.noise_std[i] for p in plist], mX[i])
        assert np.all(st == 0)
        rows.append(gps)
    cand = api.Candidates(Xs)
    b = best_so_far(prob.acquisition.fitness, data.Y, prob.y_max)
    mask = in_bounds(Xs, prob.domain.bounds) & in_cons(Xs, prob.domain.cons)
    want = api.acq_ei([[rows[i][s] for i in range(P)] for s in range(4)], cand, [1.0, 0.3], prob.y_max, b, mask, mXs)
    assert np.array_equal(acq, want[0]) and am == want[1] and mx == want[2]
    cand.close()
    for p in posts:
        p.close()
    for r in rows:
        for g in r:
            g.close()


@pytest.mark.parametrize("S", [1, 3])
def test_gradient_maximiser_equals_the_api_fed_the_device_arrays(api, plumbing, S):
    from boss_jl_amd.maximizer import posteriors_of
    from boss_jl_amd.problem import best_so_far, in_bounds, in_cons
    pl = plumbing
    B, model, data = pl["B"], pl["dev"], pl["data"]
    params = pl["plist"][0] if S == 1 else pl["plist"][:3]
    plist = [params] if S == 1 else params
    assert S == 1 or not np.array_equal(plist[0].theta, plist[1].theta)
    prob = _problem(pl, model, params)
    posts = posteriors_of(prob)
    X = np.asfortranarray(pl["Xs"][:, :17])
    am = B.HipGradientAM(x_prior=lambda r: r.uniform(0.0, 2.0, 2), multistart=4, iters=1, seed=0)
    f, g = am._value_and_grad(prob, posts, X)
    ms, _, mg = pl["dm"].program.eval_device(X, _thetas(plist), api.MEAN_SAMPLE_MAJOR, False, True)        # S×P×M, S×P×d×M
    b = best_so_far(prob.acquisition.fitness, data.Y, prob.y_max)
    mask = in_bounds(X, prob.domain.bounds) & in_cons(X, prob.domain.cons)
    gps = [[s.gp for s in p.slices] for p in posts]
    if S == 1:
        wf, wg = api.acq_ei_grad(gps[0], X, [1.0, 0.3], prob.y_max, b, mask, ms[0], mg[0])
    else:
        wf, wg = api.acq_ei_grad_set(gps, X, [1.0, 0.3], prob.y_max, b, mask, ms, mg)
    assert np.array_equal(f, wf) and np.array_equal(g, wg) and np.abs(mg).max() > 0.1
    for p in posts:
        p.close()


# ------------------------------------------------------------------------------------------ the closure is never called
def test_the_closure_is_not_called_after_tracing(B):
    rng = np.random.default_rng(31)
    d, N, P = 2, 30, 2
    X = rng.uniform(0, 2, (d, N))
    truth = np.array([0.8, -0.6, 1.3])
    Y = np.stack([[_pl(X[:, j], truth)[i] for j in range(N)] for i in range(P)]) + 0.05 * rng.standard_normal((P, N))
    tp = [B.Normal(0.0, 2.0), B.Normal(0.0, 2.0), B.Normal(1.0, 1.0)]
    counted = Counted(_pl)
    model = B.HipGaussianProcess(parametric=B.DeviceMean(counted, d, 3, P), theta_priors=tp, **_priors(B, P, d))
    traced = counted.n
    assert traced >= 9                                            # the trace and its 8 check points
    dom = B.Domain((np.zeros(d), 2 * np.ones(d)))
    prob = B.BossProblem(None, dom, B.ExpectedImprovement(B.LinFitness([1.0, 0.3])), model, B.ExperimentData(X, Y), y_max=[np.inf, 1.5])
    fit = B.HipGradientMAP(multistart=4, iters=5, seed=3).estimate_parameters(prob)
    assert np.isfinite(fit.loglike) and counted.n == traced
    prob.params = fit.params
    pts = np.asfortranarray(rng.uniform(0, 2, (d, 200)))
    for fused in (True, False):
        x, v = B.HipBatchAM(points=pts, fused=fused).maximize_acquisition(prob)
        assert np.isfinite(v) and counted.n == traced
    xs, _ = B.HipSequentialBatchAM(B.HipBatchAM(points=pts), 3).maximize_acquisition(prob)
    assert xs.shape == (d, 3) and counted.n == traced
    xs2, _ = B.HipSequentialBatchAM(B.HipBatchAM(x_prior=lambda r: r.uniform(0.0, 2.0, d), samples=50), 2).maximize_acquisition(prob)
    assert xs2.shape == (d, 2) and counted.n == traced            # the untracked path: mean(post, x) through mean_values
    x, v = B.HipGradientAM(x_prior=lambda r: r.uniform(0.0, 2.0, d), multistart=16, iters=5, seed=1).maximize_acquisition(prob)
    assert np.isfinite(v) and counted.n == traced
    # one output, one parameter set: the fused update + acquisition call (boss_gp_update_acq)
    c1 = Counted(lambda x, th: [th[0] + th[1] * x[0] + np.cos(th[2] * x[1])])
    m1 = B.HipGaussianProcess(parametric=B.DeviceMean(c1, d, 3, 1), theta_priors=tp, **_priors(B, 1, d))
    t1 = c1.n
    p1 = B.BossProblem(None, dom, B.ExpectedImprovement(B.LinFitness([1.0])), m1, B.ExperimentData(X, Y[:1]),
                       params=B.HipGPParams(np.full((d, 1), 0.5), [0.4], [0.05], truth))
    assert B.HipBatchAM._fusable(p1)
    (xa, va), (xb, vb) = (B.HipBatchAM(points=pts, fused=f).maximize_acquisition(p1) for f in (True, False))
    assert c1.n == t1 and np.isfinite(va) and np.isfinite(vb)
    # the plain closure IS called by the same paths (the counter is live)
    plain = Counted(_pl)
    prob2 = B.BossProblem(None, dom, B.ExpectedImprovement(B.LinFitness([1.0, 0.3])),
                          B.HipGaussianProcess(parametric=plain, theta_priors=tp, **_priors(B, P, d)), B.ExperimentData(X, Y),
                          y_max=[np.inf, 1.5], params=fit.params)
    B.HipBatchAM(points=pts[:, :5]).maximize_acquisition(prob2)
    assert plain.n > 0


# ------------------------------------------------------------------------------------------ the acquisition gradient without mean_grad
def test_acquisition_gradient_is_correct_without_mean_grad(B):
    """Semiparametric model M2 (d = 1), N = 30, 8 points strictly inside the bounds: HipGradientAM._value_and_grad against central
    differences of its own value, h = 1e-5, bound 1e-6·max(1, max|∇acq|) (h² truncation plus about 1e-12 / h rounding: the bound of
    test_handles_gradient_two_ways).  The plain closure without mean_grad misses the same bound: the inputs exercise ∂m/∂x."""
    from boss_jl_amd.maximizer import posteriors_of
    f, d, T, P = cases.M["M2"]
    rng = np.random.default_rng(41)
    N = 30
    X = rng.uniform(0, 20, (1, N))
    th = np.array([0.15, 15.0])
    Y = np.stack([[np.asarray(f(X[:, j], th), float)[i] for j in range(N)] for i in range(P)]) + 0.05 * rng.standard_normal((P, N))
    params = B.HipGPParams(np.full((1, P), 1.0), [1.0, 1.0], [0.1, 0.1], th)
    pri = dict(lengthscale_priors=[None] * P, amplitude_priors=[None] * P, noise_std_priors=[None] * P, theta_priors=[None] * T)
    Xq = np.asfortranarray(rng.uniform(1.0, 19.0, (1, 8)))
    h = 1e-5
    errs = {}
    for label, par in (("device", B.DeviceMean(f, d, T, P)), ("closure", f)):
        prob = B.BossProblem(None, B.Domain((np.zeros(1), 20 * np.ones(1))), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])),
                             B.HipGaussianProcess(parametric=par, **pri), B.ExperimentData(X, Y), y_max=[np.inf, 5.0], params=params)
        posts = posteriors_of(prob)
        am = B.HipGradientAM(x_prior=lambda r: r.uniform(0.0, 20.0, 1), multistart=4, iters=1, seed=0)
        a, g = am._value_and_grad(prob, posts, Xq)
        up, _ = am._value_and_grad(prob, posts, np.asfortranarray(Xq + h))
        dn, _ = am._value_and_grad(prob, posts, np.asfortranarray(Xq - h))
        for p in posts:
            p.close()
        fd = (up - dn) / (2 * h)
        errs[label] = (np.abs(g[0] - fd).max(), 1e-6 * max(1.0, np.abs(fd).max()))
        print(f"[mean-gpu] {label}: max|grad - central differences| {errs[label][0]:.3e} (bound {errs[label][1]:.3e}, max|grad| {np.abs(fd).max():.3e}, "
              f"acq in [{a.min():.3e}, {a.max():.3e}])")
    assert errs["device"][0] <= errs["device"][1]
    assert not errs["closure"][0] <= errs["closure"][1]


# ------------------------------------------------------------------------------------------ against the closure path
def test_device_mean_model_agrees_with_the_closure_model(api, plumbing):
    """The DeviceMean model against the same model with the plain closure and its exact parametric_jac: likelihoods, all gradient
    groups, μ, σ² and EI at 100 candidates, with the bound tests/test_gpu_semipar_llgrad.py holds that path to:
    tol = max(1e-9, cond(K)·N·2⁻⁵³·8), error <= 100·tol·(1 + max|want|); cond(K) from the oracle's kernel matrix of every set."""
    from boss_jl_amd.maximizer import acquisition_values
    from oracle import gp_oracle as O
    pl = plumbing
    dev, host, data, plist, P, N, Xs = pl["dev"], pl["host"], pl["data"], pl["plist"], pl["P"], pl["N"], pl["Xs"]
    cond = 0.0
    for p in plist:
        for i in range(P):
            h = O.finite_gp_params(dev.kernel, data.X.shape[0], p.lengthscales[:, i], p.amplitudes[i], p.noise_std[i])
            K = O.kernelmatrix(h, data.X)
            K[np.diag_indices(N)] += h.noise_std ** 2
            ev = np.linalg.eigvalsh(K)                            # (symmetric positive definite: cond = λmax / λmin)
            cond = max(cond, ev[-1] / ev[0])
    tol = max(1e-9, cond * N * 2.0 ** -53 * 8)

    def check(label, got, want):
        got, want = np.asarray(got, float), np.asarray(want, float)
        err, bar = np.abs(got - want).max(), 100 * tol * (1 + np.abs(want).max())
        print(f"[mean-gpu] closure path, {label}: max|d| {err:.3e} (bar {bar:.3e}, cond {cond:.3e})")
        assert err <= bar, label

    ld, gd = dev.data_loglike_grad_batch(data, plist)
    lh, gh = host.data_loglike_grad_batch(data, plist)
    check("loglike", ld, lh)
    check("loglike (values call)", dev.data_loglike_batch(data, plist), host.data_loglike_batch(data, plist))
    for name in ("lengthscales", "amplitudes", "noise_std", "theta"):
        check("d/d" + name, np.stack([getattr(g, name) for g in gd]), np.stack([getattr(g, name) for g in gh]))
    pd, ph = dev.model_posterior(plist[0], data), host.model_posterior(plist[0], data)
    (mud, vard), (muh, varh) = pd.mean_and_var(Xs), ph.mean_and_var(Xs)
    check("mu", mud, muh)
    check("var", vard, varh)
    ad = acquisition_values(_problem(pl, dev, plist[0]), [pd], Xs)[0]
    ah = acquisition_values(_problem(pl, host, plist[0]), [ph], Xs)[0]
    check("EI", ad, ah)
    assert ah.max() > 0
    pd.close()
    ph.close()
