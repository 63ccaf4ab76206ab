"""Fitness programs on the host (no GPU): tracing of closures into api.FitnessProgram, the library's interpreter and reverse sweep
(boss_fit_eval_host — the function the kernels call), validation of boss_fit_create, DeviceFitness's refusals, and a Monte-Carlo sanity
check of the numpy interpreter against the analytic LinFitness EI (so the inputs of tests/test_gpu_fitness_mc.py are known good)."""
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitness_mc_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd
    return boss_jl_amd


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F5", "F6"])
def test_traced_program_matches_closure_and_its_derivative(B, name):
    f, P = cases.F[name]
    prog = B.DeviceFitness(f, P).program
    Y = np.random.default_rng(7).standard_normal((P, 100))
    want = np.array([float(f(Y[:, k])) for k in range(100)])
    got = prog.eval(Y)
    assert np.all(np.abs(got - want) <= 1e-14 * np.maximum(1.0, np.abs(want)))
    fh, dfh = prog.eval_host(Y, want_grad=True)
    assert np.all(np.abs(fh - got) <= 1e-14 * np.maximum(1.0, np.abs(got)))
    g = prog.grad(Y)
    scale = np.abs(g).max()
    assert np.abs(g - dfh).max() <= 1e-13 * max(1.0, scale)
    # central differences, h = 1e-6: truncation ~h² plus rounding ~1e-16/h ≈ 1e-10, held to 1e-6 relative to max|∇f|
    h = 1e-6
    fd = np.stack([(prog.eval(Y + h * np.eye(P)[:, [p]]) - prog.eval(Y - h * np.eye(P)[:, [p]])) / (2 * h) for p in range(P)])
    assert np.abs(fd - g).max() <= 1e-6 * scale
    assert np.abs(fd - dfh).max() <= 1e-6 * scale


PINNED = ["F1", "F2", "F3", "F4", "F5", "G1", "W3g", "W3v", "W2v", "BIG"]


@pytest.mark.parametrize("name", PINNED)
def test_derivative_against_50_digit_central_differences(B, name):
    """An independent pin of the reverse sweep: FitnessProgram.grad was written rule for rule from the C sweep, so a rule wrong the same
    way in both passes every comparison between them.  Here df/dy comes from central differences of a forward-only mpmath interpreter
    (50 digits, h = 1e-20: error ~1e-30), at 20 standard-normal points, none within 1e-6 of a kink of ABS / MIN / MAX (asserted).
    Bound: 1e-13 · max(1, max|∇f|), the one numpy grad and eval_host are held to against each other.
    Observed max|grad - mp| = max|eval_host - mp| (bound): F1 0 (1e-13), F2 2.2e-16 (4.2e-13), F3 0 (1e-13, nearest kink 7.9e-2),
    F4 8.9e-16 (9.6e-13, nearest kink 9.3e-2), F5 5.6e-17 (1e-13), G1 2.2e-16 (1.0e-13), W3g 2.2e-16 (1.6e-13), W3v 5.6e-17 (1e-13),
    W2v 2.8e-17 (1e-13), BIG 2.2e-16 (1e-13)."""
    if name == "BIG":
        prog = cases.big_program(B.api)
        assert prog.code.shape[0] == B.api.FIT_MAX_INSTR and prog.consts.shape[0] == B.api.FIT_MAX_CONSTS and prog.P == B.api.FIT_MAX_INPUTS
        read = set(prog.code[:, 1]) | set(prog.code[:, 2])
        assert set(range(prog.P + prog.consts.shape[0])) <= read                      # every input and every constant is read
        ids, uses = np.unique(prog.code[:, 1:], return_counts=True)
        assert uses[ids >= prog.P + prog.consts.shape[0]].max() >= 3                  # an adjoint that accumulates
    else:
        f, P = cases.F[name]
        prog = B.DeviceFitness(f, P).program
    Y = np.random.default_rng(21).standard_normal((prog.P, 20))
    ref, kink = cases.mp_grad(prog, Y)
    assert kink >= 1e-6, kink
    g = prog.grad(Y)
    _, dfh = prog.eval_host(Y, want_grad=True)
    tol = 1e-13 * max(1.0, np.abs(ref).max())
    print(f"{name}: max|grad - mp| = {np.abs(g - ref).max():.3e}, max|eval_host - mp| = {np.abs(dfh - ref).max():.3e} (tol {tol:.3e}), "
          f"nearest kink {kink:.3e}")
    assert np.abs(g - ref).max() <= tol
    assert np.abs(dfh - ref).max() <= tol


def test_the_closures_reach_every_workgroup_shape(B):
    """The launch rule of the Monte-Carlo kernels on the traced programs: each kernel runs with 1, 2, 3 and 4 waves somewhere (the
    device tests pick their programs by this; a closure that changes size cannot lose a shape silently)."""
    for grad in (False, True):
        seen = set()
        for f, P in cases.F.values():
            prog = B.DeviceFitness(f, P).program
            seen.add(cases.mc_waves(prog.P, prog.code.shape[0], grad))
        assert seen == {1, 2, 3, 4}, (grad, seen)


def _one(api, op, x, z=None, const_b=False):
    """(value, d/da, d/db) of one instruction through boss_fit_eval_host."""
    name = api.FIT_OP[op]
    if z is None:
        p = api.FitnessProgram(1, [], [[name, 0, -1]], 1)
        f, df = p.eval_host(np.array([x]), want_grad=True)
        return f, df[0], None
    if const_b:
        p = api.FitnessProgram(1, [z], [[name, 0, 1]], 2)
        f, df = p.eval_host(np.array([x]), want_grad=True)
        return f, df[0], None
    p = api.FitnessProgram(2, [], [[name, 0, 1]], 2)
    f, df = p.eval_host(np.array([x, z]), want_grad=True)
    return f, df[0], df[1]


def test_every_opcode_alone_at_edge_inputs(api):
    assert _one(api, "ADD", 1.5, 2.0) == (3.5, 1.0, 1.0)
    assert _one(api, "SUB", 1.5, 2.0) == (-0.5, 1.0, -1.0)
    assert _one(api, "MUL", 1.5, 2.0) == (3.0, 2.0, 1.5)
    assert _one(api, "DIV", 3.0, 2.0) == (1.5, 0.5, -0.75)
    assert _one(api, "NEG", 1.5)[:2] == (-1.5, -1.0)
    assert _one(api, "ABS", -1.5)[:2] == (1.5, -1.0)
    assert _one(api, "ABS", 0.0)[:2] == (0.0, 0.0)                  # ABS'(0) = 0
    assert _one(api, "SQUARE", -3.0)[:2] == (9.0, -6.0)
    assert _one(api, "SQRT", 4.0)[:2] == (2.0, 0.25)
    f, da, _ = _one(api, "SQRT", 0.0)
    assert f == 0.0 and da == np.inf                               # as IEEE gives
    assert _one(api, "EXP", 0.0)[:2] == (1.0, 1.0)
    assert _one(api, "LOG", 1.0)[:2] == (0.0, 1.0)
    assert math.isnan(_one(api, "LOG", -1.0)[0])
    f, da, _ = _one(api, "SIN", 0.3)
    assert abs(f - math.sin(0.3)) <= 1e-16 and abs(da - math.cos(0.3)) <= 1e-16
    f, da, _ = _one(api, "COS", 0.3)
    assert abs(f - math.cos(0.3)) <= 1e-16 and abs(da + math.sin(0.3)) <= 1e-16
    f, da, _ = _one(api, "TANH", 0.3)
    assert abs(f - math.tanh(0.3)) <= 1e-16 and abs(da - (1 - math.tanh(0.3) ** 2)) <= 2e-16
    assert _one(api, "POW", -2.0, 3.0, const_b=True)[:2] == (-8.0, 12.0)       # constant exponent: no log(a) term, no NaN
    f, da, db = _one(api, "POW", 2.0, 3.0)
    assert f == 8.0 and da == 12.0 and abs(db - 8.0 * math.log(2.0)) <= 1e-15
    assert _one(api, "MIN", 1.0, 2.0) == (1.0, 1.0, 0.0) and _one(api, "MIN", 2.0, 1.0) == (1.0, 0.0, 1.0)
    assert _one(api, "MAX", 1.0, 2.0) == (2.0, 0.0, 1.0) and _one(api, "MAX", 2.0, 1.0) == (2.0, 1.0, 0.0)
    assert _one(api, "MIN", 1.0, 1.0) == (1.0, 1.0, 0.0) and _one(api, "MAX", 1.0, 1.0) == (1.0, 1.0, 0.0)   # ties: the first operand
    assert math.isnan(_one(api, "MIN", float("nan"), 1.0)[0]) and math.isnan(_one(api, "MAX", 1.0, float("nan"))[0])
    # the value may be an input or a constant
    assert api.FitnessProgram(2, [4.0], [], 1).eval_host(np.array([1.0, 2.0])) == 2.0
    f, df = api.FitnessProgram(2, [4.0], [], 2).eval_host(np.array([1.0, 2.0]), want_grad=True)
    assert f == 4.0 and np.all(df == 0.0)


def test_malformed_programs_are_refused(api):
    ADD, SIN = api.FIT_OP["ADD"], api.FIT_OP["SIN"]
    bad = {
        "forward reference": (2, [], [[ADD, 0, 3], [ADD, 0, 1]], 3),
        "self reference": (2, [], [[ADD, 0, 2]], 2),
        "unknown opcode": (2, [], [[16, 0, 1]], 2),
        "negative opcode": (2, [], [[-1, 0, 1]], 2),
        "too many inputs": (17, [], [], 0),
        "too many constants": (1, [1.0] * 33, [], 0),
        "too many instructions": (1, [], [[SIN, i, -1] for i in range(65)], 65),
        "non-finite constant": (1, [float("inf")], [], 0),
        "NaN constant": (1, [float("nan")], [], 0),
        "b on a unary op": (2, [], [[SIN, 0, 1]], 2),
        "missing b": (2, [], [[ADD, 0, -1]], 2),
        "bad out_id": (2, [], [[ADD, 0, 1]], 3),
    }
    for why, (P, consts, code, out) in bad.items():
        with pytest.raises(api.BossError) as e:
            api.FitnessProgram(P, consts, np.asarray(code, dtype=np.intc).reshape(-1, 3), out)
        assert e.value.code == api.BOSS_E_INVALID, why
        assert len(str(e.value)) > 25, why                       # a message, not just the code
    api.FitnessProgram(1, [], [[SIN, i, -1] for i in range(64)], 64)     # the limit itself is fine


def test_device_fitness_refuses_what_it_cannot_trace(B):
    def chain(y):
        f = y[0]
        for _ in range(65):
            f = np.sin(f)
        return f
    for f, P, word in [(lambda y: y[0] if y[1] > 0 else 0.0, 2, "compares"), (lambda y: math.sin(y[0]), 2, "float"),
                       (lambda y: np.arctan(y[0]), 2, "arctan"), (chain, 1, "65 instructions"), (lambda y: y[0], 17, "y_dim = 17")]:
        with pytest.raises(ValueError) as e:
            B.DeviceFitness(f, P)
        assert word in str(e.value)
    # a trace that hides a branch from the tracer is caught by the check against the closure
    state = {"n": 0}

    def moody(y):
        state["n"] += 1
        return y[0] if state["n"] == 1 else 2.0 * y[0]
    with pytest.raises(ValueError) as e:
        B.DeviceFitness(moody, 1)
    assert "disagrees" in str(e.value)


def test_device_fitness_is_a_nonlin_fitness(B):
    f, P = cases.F["F1"]
    dfit = B.DeviceFitness(f, P)
    assert isinstance(dfit, B.NonlinFitness)
    y = np.array([0.3, -0.7])
    assert dfit(y) == float(f(y))
    # the whole-vector forms of the tracer
    g = B.DeviceFitness(lambda y: np.sin(y).sum() + y @ np.arange(3.0) + np.dot(y, [1.0, 2.0, 3.0]) + abs(y[1]) + np.square(y[2])
                        + np.power(y[0], 3) + np.maximum(y, 0.0).sum() + (2.0 / (1.0 + np.exp(-y[:2]))).sum(), 3)
    Y = np.random.default_rng(3).standard_normal((3, 20))
    want = np.array([g(Y[:, k]) for k in range(20)])
    assert np.all(np.abs(g.program.eval(Y) - want) <= 1e-14 * np.maximum(1.0, np.abs(want)))


def test_monte_carlo_of_the_linear_program_matches_the_analytic_ei(B):
    """64 candidates, F6, K = 4096: the numpy Monte-Carlo EI from program.eval within 6 σ_f / sqrt(K) of the analytic LinFitness EI.
    (The standard deviation of max(0, X) is at most that of X, which is σ_f.)"""
    from scipy.special import erfc
    f, P = cases.F["F6"]
    prog = B.DeviceFitness(f, P).program
    M, K, best = 64, 4096, 0.1
    mu, var = cases.moments(11, 1, P, M)
    eps = cases.eps_for(12, 1, P, K)
    fv = cases.f_values(prog, mu, var, eps)[0]
    mc = np.maximum(0.0, fv - best).mean(1)
    c = np.array([0.7, -0.2])
    muf, sf = c @ mu[0], np.sqrt((c * c) @ var[0])
    z = (muf - best) / sf
    ei = (muf - best) * 0.5 * erfc(-z / math.sqrt(2.0)) + sf * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    assert np.all(np.abs(mc - ei) <= 6.0 * sf / math.sqrt(K))
