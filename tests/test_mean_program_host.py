"""Mean programs without a device: the tracer (B.DeviceMean / trace_mean), api.MeanProgram's numpy interpreter and the library's host
interpreter (boss_mean_eval_host: the functions the kernel calls), the two layouts, and every refusal.

Values: the program against the closure at 100 random (x, θ), to 1e-14·max(1, |m|).  Jacobians: ∂m/∂θ and ∂m/∂x from the numpy sweep
and from boss_mean_eval_host against central differences of a 50-digit forward interpreter (fitness_mc_cases.mp_grad, h = 1e-20: no
differentiation rule enters the truth), to 1e-13·max(1, max|∇|) — the bound the fitness sweep is held to."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitness_mc_cases as fcases  # noqa: E402
import mean_program_cases as cases  # noqa: E402

NAMES = ["M1", "M2", "M3", "M4", "M5", "M6"]
KINK_SEED = {"M1": 11, "M2": 11, "M3": 11, "M4": 11, "M5": 11, "M6": 11}      # seeds whose 20 points stay 1e-6 away from every kink (asserted)


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def means(B):
    out = {name: B.DeviceMean(*spec) for name, spec in cases.M.items()}
    out["M6"] = cases.HandMean(cases.big_mean_program(B.api))
    return out


def test_the_cases_are_what_they_claim(means):
    m6 = means["M6"].program
    assert (m6.d, m6.T, m6.P) == (16, 16, 2)
    big = m6.outputs[0]
    assert big.code.shape[0] == 64 and big.consts.shape[0] == 32
    read = set(big.code[:, 1]) | set(big.code[:, 2])
    assert set(range(64)) <= read                                 # all 32 inputs and all 32 constants are read
    m3 = means["M3"].program
    assert m3.outputs[2].code.shape[0] == 0 and list(m3.outputs[2].consts) == [1.5]          # the constant output
    assert means["M5"].program.T == 0
    assert means["T1"].program.outputs[0].code.shape[0] == 3


@pytest.mark.parametrize("name", NAMES)
def test_values_match_the_closure_and_the_host_interpreter(means, name):
    dm = means[name]
    prog = dm.program
    X, Th = cases.points(3, prog.d, prog.T, 100, 100)
    with np.errstate(all="ignore"):
        want = np.array([np.asarray(dm(X[:, k], Th[:, k]) if prog.T else dm(X[:, k]), float).reshape(-1) for k in range(100)])    # 100×P
    got = np.array([prog.eval(X[:, k], None if Th is None else Th[:, k])[0, :, 0] for k in range(100)])
    host = np.array([prog.eval_host(X[:, k], None if Th is None else Th[:, k])[0][0, :, 0] for k in range(100)])
    bound = 1e-14 * np.maximum(1.0, np.abs(want))
    print(f"[mean-host] {name}: max|program - closure| {np.abs(got - want).max():.3e}, max|eval_host - program| {np.abs(host - got).max():.3e}")
    assert np.all(np.abs(got - want) <= bound)
    assert np.all(np.abs(host - got) <= 1e-14 * np.maximum(1.0, np.abs(got)))
    # all sets against all points in one call equals point by point
    m_all = prog.eval_host(X[:, :7], None if Th is None else Th[:, :3])[0]
    for s in range(m_all.shape[0]):
        for j in range(7):
            assert np.array_equal(m_all[s, :, j], prog.eval_host(X[:, j], None if Th is None else Th[:, s])[0][0, :, 0])


@pytest.mark.parametrize("name", NAMES)
def test_jacobians_match_50_digit_central_differences(means, name):
    prog = means[name].program
    d, T, P, n = prog.d, prog.T, prog.P, 20
    X, Th = cases.points(KINK_SEED[name], d, T, n, n)             # point k takes its own θ_k
    Y = X if Th is None else np.vstack([X, Th])                   # (d + T)×n: the shared input vector
    truth, kink = [], math.inf
    for q in prog.outputs:
        g, kq = fcases.mp_grad(q, Y)
        truth.append(g)
        kink = min(kink, kq)
    truth = np.stack(truth)                                       # P×(d + T)×n
    print(f"[mean-host] {name}: nearest kink {kink:.3e}")
    assert kink > 1e-6
    jt_np = np.zeros((P, n, T))
    jx_np = np.zeros((P, d, n))
    jt_h, jx_h = np.zeros((P, n, T)), np.zeros((P, d, n))
    for k in range(n):
        th = None if Th is None else Th[:, k]
        jt, jx = prog.jac(X[:, k], th)
        _, jth, jxh = prog.eval_host(X[:, k], th, 0, T > 0, True)
        jx_np[:, :, k], jx_h[:, :, k] = jx[0, :, :, 0], jxh[0, :, :, 0]
        if T:
            jt_np[:, k, :], jt_h[:, k, :] = jt[0, :, 0, :], jth[0, :, 0, :]
    want_x, want_t = truth[:, :d, :], truth[:, d:, :].transpose(0, 2, 1)
    bound = 1e-13 * max(1.0, np.abs(truth).max())
    for label, got, want in (("numpy d/dx", jx_np, want_x), ("numpy d/dtheta", jt_np, want_t), ("host d/dx", jx_h, want_x),
                             ("host d/dtheta", jt_h, want_t)):
        err = np.abs(got - want).max() if want.size else 0.0
        print(f"[mean-host] {name} {label}: max err {err:.3e} (bound {bound:.3e}, max|grad| {np.abs(truth).max():.3e})")
        assert err <= bound


@pytest.mark.parametrize("n", [1, 65])
def test_both_layouts_follow_the_index_formulas(means, n):
    prog = means["M2"].program
    S, P, d, T = 3, 2, prog.d, prog.T
    X, Th = cases.points(5, d, T, n, S)
    m = prog.eval(X, Th)                                          # S×P×n
    jt, jx = prog.jac(X, Th)                                      # S×P×n×T, S×P×d×n
    for layout in (0, 1):
        mh, jth, jxh = prog.eval_host(X, Th, layout, True, True)
        fm = np.ascontiguousarray(mh).ravel()
        ft = np.ascontiguousarray(jth.transpose(0, 1, 3, 2)).ravel()              # back to the order of the memory the C ABI filled
        fx = np.ascontiguousarray(jxh.transpose(0, 1, 3, 2)).ravel()
        assert jth.transpose(0, 1, 3, 2).flags.c_contiguous and jxh.transpose(0, 1, 3, 2).flags.c_contiguous
        for s in range(S):
            for p in range(P):
                blk = p + P * s if layout == 0 else s + S * p
                for j in range(n):
                    assert abs(fm[blk * n + j] - m[s, p, j]) <= 1e-14 * max(1.0, abs(m[s, p, j]))
                    for t in range(T):
                        assert abs(ft[blk * n * T + j + n * t] - jt[s, p, j, t]) <= 1e-13 * max(1.0, np.abs(jt).max())
                    for k in range(d):
                        assert abs(fx[blk * d * n + k + d * j] - jx[s, p, k, j]) <= 1e-13 * max(1.0, np.abs(jx).max())
        # the views the binding hands out
        blocks = (lambda a: a) if layout == 0 else (lambda a: a.swapaxes(0, 1))
        assert blocks(mh).shape == (S, P, n) and blocks(jth).shape == (S, P, n, T) and blocks(jxh).shape == (S, P, d, n)
    only_t = prog.eval_host(X, Th, 0, True, False)
    only_x = prog.eval_host(X, Th, 0, False, True)
    assert only_t[2] is None and only_x[1] is None and np.array_equal(only_t[1], prog.eval_host(X, Th, 0, True, True)[1])
    assert np.array_equal(only_x[2], prog.eval_host(X, Th, 0, True, True)[2])


# ------------------------------------------------------------------------------------------ refusals
def _nest(v, k):
    """sin applied k times: k instructions, no constant."""
    for _ in range(k):
        v = np.sin(v)
    return v


def test_trace_mean_refusals(B):
    import math as pymath
    DM = B.DeviceMean
    bad = {
        "branch": (lambda x, th: [x[0] if x[0] > 0 else th[0]], 1, 1, 1, "compares"),
        "bool": (lambda x, th: [x[0] if x[0] else th[0]], 1, 1, 1, "branches"),
        "math": (lambda x, th: [pymath.sin(x[0]) + th[0]], 1, 1, 1, "float"),
        "float": (lambda x, th: [float(x[0]) + th[0]], 1, 1, 1, "float"),
        "length": (lambda x, th: [x[0], th[0]], 1, 1, 3, "returned 2 outputs"),
        "scalar for two": (lambda x, th: x[0] * th[0], 1, 1, 2, "list, a tuple or a vector"),
        "unsupported": (lambda x, th: [np.arctan(x[0]) + th[0]], 1, 1, 1, "arctan"),
        "instructions": (lambda x, th: [_nest(x[0], 65) + th[0]], 1, 1, 1, "instructions"),
        "constants": (lambda x, th: [sum(x[0] * (k + 1.5) for k in range(33)) + th[0]], 1, 1, 1, "constants"),
        "not finite": (lambda x, th: [x[0] * np.inf + th[0]], 1, 1, 1, "not finite"),
        "vector entry": (lambda x, th: [x, th[0]], 2, 1, 2, "must be a scalar"),
    }
    for name, (f, d, T, P, word) in bad.items():
        with pytest.raises(ValueError) as e:
            DM(f, d, T, P)
        assert str(e.value).startswith("DeviceMean:") and word in str(e.value), (name, str(e.value))
    for d, T, P in ((0, 1, 1), (20, 13, 1), (1, -1, 1), (1, 1, 0), (1, 1, 17)):
        with pytest.raises(ValueError) as e:
            DM(lambda x, th: [x[0]] * max(P, 1), d, T, P)
        assert str(e.value).startswith("DeviceMean:")
    # something the trace cannot see: the check against the closure at 8 points catches it
    calls = {"n": 0}

    def sneaky(x, th):
        calls["n"] += 1
        return [x[0] * th[0] + (0.0 if calls["n"] == 1 else 1.0)]
    with pytest.raises(ValueError) as e:
        DM(sneaky, 1, 1, 1)
    assert "disagrees with the closure" in str(e.value)
    # the fitness tracer keeps its own voice
    with pytest.raises(ValueError) as e:
        B.DeviceFitness(lambda y: np.arctan(y[0]), 1)
    assert str(e.value).startswith("DeviceFitness:") and "device fitness" in str(e.value)
    # accepted return types: list, tuple, traced vector, numpy object array, constant entries
    for f in (lambda x, th: (x[0] * th[0], 2.0), lambda x, th: x * th[0], lambda x, th: np.array([x[0] * th[0], x[1]]),
              lambda x, th: [th[0], 0.0]):
        assert DM(f, 2, 1, 2).program.P == 2


def test_mean_create_refusals(api):
    op = api.FIT_OP
    ok = ([0.5], [(op["MUL"], 0, 2)], 3)                          # d = 1, T = 1: ids 0 x, 1 θ, 2 constant, 3 the product
    api.MeanProgram(1, 1, [ok, ok]).close()
    bad = {
        "forward reference": ([0.5], [(op["MUL"], 0, 3)], 3),
        "self reference a": ([0.5], [(op["NEG"], 3, -1)], 3),
        "unknown opcode": ([0.5], [(16, 0, 1)], 3),
        "negative opcode": ([0.5], [(-1, 0, 1)], 3),
        "unary with b": ([0.5], [(op["SIN"], 0, 1)], 3),
        "binary without b": ([0.5], [(op["ADD"], 0, -1)], 3),
        "bad out_id": ([0.5], [(op["MUL"], 0, 2)], 4),
        "negative out_id": ([0.5], [(op["MUL"], 0, 2)], -1),
        "nan constant": ([np.nan], [(op["MUL"], 0, 2)], 3),
        "inf constant": ([np.inf], [(op["MUL"], 0, 2)], 3),
        "33 constants": (list(np.arange(33.0)), [], 0),
        "65 instructions": ([], [(op["NEG"], 0, -1)] * 65, 2),
    }
    for name, prog in bad.items():
        with pytest.raises(api.BossError) as e:
            api.MeanProgram(1, 1, [ok, prog])
        assert e.value.code == api.BOSS_E_INVALID and "output 1:" in str(e.value), (name, str(e.value))
        if "reference" in name or "opcode" in name or "with" in name:
            assert "instruction 0:" in str(e.value), (name, str(e.value))
    for d, T, outs in ((0, 1, [ok]), (1, -1, [ok]), (17, 16, [ok]), (1, 1, []), (1, 1, [ok] * 17)):
        with pytest.raises(api.BossError) as e:
            api.MeanProgram(d, T, outs)
        assert e.value.code == api.BOSS_E_INVALID
    lib = api.load_library()
    assert lib.boss_mean_create(1, 1, 1, None, None, None, None, None, None) == api.BOSS_E_INVALID
    h = C.c_void_p()
    assert lib.boss_mean_create(1, 1, 1, None, None, None, None, None, C.byref(h)) == api.BOSS_E_INVALID and not h
    lib.boss_mean_free(None)


def test_eval_refusals(api, means):
    lib = api.load_library()
    prog, p0 = means["M2"].program, means["M5"].program
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))        # noqa: E731
    X, th, out = np.zeros((3, 4)), np.zeros((2, 4)), np.zeros(4096)
    for fn, head in ((lib.boss_mean_eval_host, ()), (lib.boss_mean_eval, (0,))):
        call = lambda *a: fn(*head, *a)                           # noqa: E731
        assert call(None, 4, dp(X), 1, dp(th), 0, dp(out), None, None) == api.BOSS_E_INVALID
        assert call(prog._h, 0, dp(X), 1, dp(th), 0, dp(out), None, None) == api.BOSS_E_INVALID
        assert call(prog._h, 4, dp(X), 0, dp(th), 0, dp(out), None, None) == api.BOSS_E_INVALID
        assert call(prog._h, 4, None, 1, dp(th), 0, dp(out), None, None) == api.BOSS_E_INVALID
        assert call(prog._h, 4, dp(X), 1, dp(th), 0, None, None, None) == api.BOSS_E_INVALID
        assert call(prog._h, 4, dp(X), 1, None, 0, dp(out), None, None) == api.BOSS_E_INVALID              # T > 0 without thetas
        assert call(p0._h, 1, dp(X), 1, None, 0, dp(out), dp(out), None) == api.BOSS_E_INVALID             # jac_theta with T == 0
        for layout in (-1, 2):
            assert call(prog._h, 4, dp(X), 1, dp(th), layout, dp(out), None, None) == api.BOSS_E_INVALID
        # P·S·n·max(1, T, d) above 2^30: P = 2, T = 2 (refused before anything is read)
        assert call(prog._h, (1 << 28) + 1, dp(X), 1, dp(th), 0, dp(out), None, None) == api.BOSS_E_INVALID
        assert call(prog._h, 1 << 14, dp(X), 1 << 15, dp(th), 0, dp(out), None, None) == api.BOSS_E_INVALID
        assert b"2^30" in lib.boss_last_error()
    assert lib.boss_mean_eval_host(p0._h, 1, dp(X), 1, None, 0, dp(out), None, dp(out[8:])) == api.BOSS_OK   # T = 0, NULL thetas: fine
    with pytest.raises(api.BossError):
        p0.eval_host(X, None, 0, True, False)
    with pytest.raises(api.BossError):
        prog.eval_host(np.zeros((1, 2)), np.zeros((2, 1)), 2)
    with pytest.raises(ValueError):
        prog.eval_host(np.zeros((2, 2)), np.zeros((2, 1)))


def test_device_call_without_a_device(api, means):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(api.BossError) as e:
        means["M2"].program.eval_device(np.zeros((1, 3)), np.zeros((2, 1)))
    assert e.value.code == api.BOSS_E_NO_DEVICE


def test_mean_grad_beside_a_device_mean_is_refused(B, means):
    f, d, T, P = cases.M["M4"]
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (d, 10))
    prob = B.BossProblem(f=None, domain=B.Domain(bounds=([0.] * d, [1.] * d)), y_max=[np.inf] * P,
                         acquisition=B.ExpectedImprovement(B.LinFitness([1.0, 0.0])),
                         model=B.HipGaussianProcess(lengthscale_priors=[None] * P, amplitude_priors=[None] * P, noise_std_priors=[None] * P,
                                                    parametric=means["M4"], theta_priors=[B.Normal(0.0, 1.0)] * T),
                         data=B.ExperimentData(X, rng.standard_normal((P, 10))),
                         params=B.HipGPParams(np.full((d, P), 0.4), [1.0] * P, [0.05] * P, np.array([0.3, 0.2])))
    am = B.HipGradientAM(x_prior=lambda r: r.uniform(0.0, 1.0, d), multistart=4, iters=1, seed=0, mean_grad=lambda x: np.zeros((P, d)))
    with pytest.raises(ValueError) as e:
        am.maximize_acquisition(prob)
    assert "DeviceMean" in str(e.value) and "mean_grad" in str(e.value)
    # and the closure is still what a host path calls
    assert np.allclose(means["M4"](X[:, 0], np.array([0.3, 0.2])), np.asarray(f(X[:, 0], np.array([0.3, 0.2])), float))
