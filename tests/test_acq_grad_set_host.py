"""Host side of boss_acq_ei_grad_set (no GPU): HipGradientAM hands the S samples of a BI fit to ONE device call, and the
expectation the GPU tests use — the mean over s of oracle.gp_oracle.ei_acquisition_grad — is the gradient of the mean of
ei_acquisition (central finite differences, step and tolerance of tests/test_oracle_crosscheck.py:142-149)."""
import types

import numpy as np

from oracle import gp_oracle as O


class _Slice:
    def __init__(self, gp, mean):
        self.gp, self.mean = gp, mean

    def _mean_s(self, X):
        return None if self.mean is None else self.mean(X)


def _stub_and_problem(monkeypatch, S, P=2, d=3, with_means=True):
    import boss_jl_amd as B
    from boss_jl_amd import maximizer as MX
    calls = []

    class GibbsGP:                                                # (what the maximiser tests handles against)
        pass

    def acq_ei_grad_set(gps, Xs, coefs, y_max, best, mask, ms, mg):
        calls.append(("set", gps, ms, mg))
        return np.zeros(Xs.shape[1]), np.zeros(Xs.shape)

    def acq_ei_grad(gps, Xs, coefs, y_max, best, mask, ms, mg):
        calls.append(("one", gps, ms, mg))
        return np.ones(Xs.shape[1]), np.ones(Xs.shape)

    monkeypatch.setattr(MX, "api", types.SimpleNamespace(GibbsGP=GibbsGP, acq_ei_grad_set=acq_ei_grad_set, acq_ei_grad=acq_ei_grad))
    means = [[(lambda X, s=s, p=p: 10.0 * s + p + X[0]) if with_means else None for p in range(P)] for s in range(S)]
    posts = [types.SimpleNamespace(slices=[_Slice(("gp", s, p), means[s][p]) for p in range(P)]) for s in range(S)]
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((P, 12))
    prob = B.BossProblem(None, B.Domain((np.zeros(d), np.ones(d))), B.ExpectedImprovement(B.LinFitness([1.0, 0.5])), None,
                         B.ExperimentData(rng.uniform(0, 1, (d, 12)), Y), [np.inf, 0.3], None)
    return B, calls, posts, prob


def test_bi_samples_make_one_set_call(monkeypatch):
    S, P, d, M = 4, 2, 3, 7
    B, calls, posts, prob = _stub_and_problem(monkeypatch, S, P, d)
    X = np.random.default_rng(1).uniform(0, 1, (d, M))
    am = B.HipGradientAM(x_prior=None, mean_grad=lambda x: np.arange(P * d, dtype=float).reshape(P, d) + x[0])
    f, g = am._value_and_grad(prob, posts, X)
    assert [c[0] for c in calls] == ["set"], calls
    _, gps, ms, mg = calls[0]
    assert [[h for h in row] for row in gps] == [[("gp", s, p) for p in range(P)] for s in range(S)]      # gps[s][p]
    assert ms.shape == (S, P, M) and mg.shape == (S, P, d, M)
    for s in range(S):
        for p in range(P):
            assert np.array_equal(ms[s, p], 10.0 * s + p + X[0])
            for j in range(M):
                assert np.array_equal(mg[s, p, :, j], np.arange(P * d, dtype=float).reshape(P, d)[p] + X[0, j])
    assert f.shape == (M,) and g.shape == (d, M)


def test_no_means_travel_as_none(monkeypatch):
    B, calls, posts, prob = _stub_and_problem(monkeypatch, 3, with_means=False)
    B.HipGradientAM(x_prior=None)._value_and_grad(prob, posts, np.zeros((3, 5)))
    assert [c[0] for c in calls] == ["set"] and calls[0][2] is None and calls[0][3] is None


def test_one_sample_keeps_the_single_call(monkeypatch):
    B, calls, posts, prob = _stub_and_problem(monkeypatch, 1)
    f, g = B.HipGradientAM(x_prior=None)._value_and_grad(prob, posts, np.zeros((3, 5)))
    assert [c[0] for c in calls] == ["one"] and calls[0][1] == [("gp", 0, 0), ("gp", 0, 1)]
    assert np.array_equal(f, np.ones(5)) and np.array_equal(g, np.ones((3, 5)))


def test_nonstationary_samples_keep_the_loop(monkeypatch):
    from boss_jl_amd import maximizer as MX
    B, calls, posts, prob = _stub_and_problem(monkeypatch, 3)
    posts[1].slices[0].gp = MX.api.GibbsGP()
    B.HipGradientAM(x_prior=None)._value_and_grad(prob, posts, np.zeros((3, 5)))
    assert [c[0] for c in calls] == ["one"] * 3


def test_python_binding_covers_the_symbol():
    from boss_jl_amd import api
    assert "boss_acq_ei_grad_set" in api.SIGNATURES and callable(api.acq_ei_grad_set) and callable(api._set_grad_launches)
    assert len(api.SIGNATURES["boss_acq_ei_grad_set"][1]) == len(api.SIGNATURES["boss_acq_ei_grad"][1]) + 1


def test_mean_of_sample_gradients_is_the_gradient_of_the_mean():
    """N = 40, d = 3, S = 3, P = 2, per-sample prior means: mean_s ei_acquisition_grad against central differences of
    mean_s ei_acquisition (eps = 1e-6, rtol 1e-5, atol 1e-8: tests/test_oracle_crosscheck.py:142-149)."""
    rng = np.random.default_rng(21)
    d, N, M, P, S = 3, 40, 9, 2, 3
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1] + 0.2 * np.cos(4 * X[2])])
    lam = rng.uniform(0.35, 0.8, (S, P, d))
    amp = rng.uniform(0.8, 1.5, (S, P))
    c = rng.uniform(-0.2, 0.2, (S, P))
    gr = rng.uniform(-0.2, 0.2, (S, P, d))
    mean = lambda s, p, Z: c[s, p] + gr[s, p] @ Z                 # noqa: E731
    posts = [[O.gp_fit(X, Y[p], "matern52", lam[s, p], amp[s, p], 0.05, mean=mean(s, p, X)) for p in range(P)] for s in range(S)]
    Xs = rng.uniform(0.05, 0.95, (d, M))
    y_max, coefs = [np.inf, 0.3], [1.0, 0.2]
    b = O.best_so_far(coefs, Y, y_max)
    ms = lambda s, Z: [mean(s, p, Z) for p in range(P)]           # noqa: E731
    mgs = lambda s: [np.repeat(gr[s, p][:, None], M, axis=1) for p in range(P)]   # noqa: E731
    avg = lambda Z, ym, bb: sum(O.ei_acquisition(posts[s], Z, coefs, ym, bb, means_s=ms(s, Z)) for s in range(S)) / S   # noqa: E731
    for ym, bb in ((y_max, b), (None, b), (y_max, None)):
        res = [O.ei_acquisition_grad(posts[s], Xs, coefs, ym, bb, means_s=ms(s, Xs), mean_grads_s=mgs(s)) for s in range(S)]
        acq, dacq = sum(r[0] for r in res) / S, sum(r[1] for r in res) / S
        assert np.allclose(acq, avg(Xs, ym, bb), rtol=0, atol=1e-14)
        eps = 1e-6
        for k in range(d):
            Xp, Xm = Xs.copy(), Xs.copy()
            Xp[k] += eps
            Xm[k] -= eps
            fd = (avg(Xp, ym, bb) - avg(Xm, ym, bb)) / (2 * eps)
            assert np.allclose(dacq[k], fd, rtol=1e-5, atol=1e-8), (ym, bb, k)
