"""Kernel programs without a device: the tracer (B.DeviceKernel / trace_kernel), api.KernelProgram's numpy interpreter and the
library's host interpreter (boss_kern_eval_host: the function the kernels call), every refusal of the tracer, and the argument checks
of boss_kern_create / boss_kgp_create.

Values: the program against the closure at 200 seeded point pairs, to 1e-14·max(1, |k|) — the tolerance
tests/test_mean_program_host.py holds its programs to."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_program_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.mark.parametrize("d", [1, 3, 16])
@pytest.mark.parametrize("name", sorted(cases.CLOSURES))
def test_values_match_the_closure_and_the_host_interpreter(B, name, d):
    f = cases.CLOSURES[name]
    dk = B.DeviceKernel(f, d)
    prog = dk.program
    assert prog.d == d and prog.code.shape[0] <= 64 and prog.consts.shape[0] <= 32
    rng = np.random.default_rng(100 + d)
    U, V = rng.standard_normal((d, 200)), rng.standard_normal((d, 200))
    want = np.array([float(dk(U[:, k], V[:, k])) for k in range(200)])     # calling a DeviceKernel calls the closure
    got, host = prog.eval(U, V), prog.eval_host(U, V)
    bound = 1e-14 * np.maximum(1.0, np.abs(want))
    print(f"[kern-host] {name} d={d}: {prog.code.shape[0]} instructions, max|program - closure| {np.abs(got - want).max():.3e}, "
          f"max|eval_host - closure| {np.abs(host - want).max():.3e}")
    assert np.all(np.abs(got - want) <= bound)
    assert np.all(np.abs(host - want) <= bound)
    # the whole-matrix forms the GPU tests restate K with are the closure
    assert np.all(np.abs(cases.pairs(f, U, V) - want) <= bound)
    G = cases.gram(f, U[:, :7], V[:, :5])
    for i in range(7):
        for j in range(5):
            assert abs(G[i, j] - float(f(U[:, i], V[:, j]))) <= 1e-14 * max(1.0, abs(G[i, j]))
    # one point pair
    assert prog.eval_host(U[:, 0], V[:, 0]) == host[0] and prog.eval(U[:, 0], V[:, 0]) == got[0]


def test_the_dot_product_kernel_has_no_constant_prior_variance(B):
    prog = B.DeviceKernel(cases.dot1, 3).program
    U = np.random.default_rng(5).standard_normal((3, 10))
    kss = prog.eval_host(U, U)
    assert np.ptp(kss) > 0.5 and np.allclose(kss, (U * U).sum(0) + 1, rtol=0, atol=1e-14 * 10)


def test_a_closure_without_inputs_is_a_constant_program(B):
    prog = B.DeviceKernel(lambda u, v: 2.5, 2).program
    assert prog.code.shape[0] == 0 and prog.eval_host(np.zeros(2), np.ones(2)) == 2.5


def _deep(x):
    for _ in range(70):                                      # 71 instructions, no constant
        x = np.sin(x)
    return x


BAD = {
    "branch": (lambda u, v: u[0] * v[0] if u[0] > 0 else 0.0, 1, "data-dependent"),
    "math": (lambda u, v: math.exp(-(u[0] - v[0]) ** 2), 1, "math"),
    "float": (lambda u, v: float(u[0]) * float(v[0]), 1, "float()"),
    "unsupported": (lambda u, v: np.arctan(u[0] * v[0]), 1, "arctan"),
    "unsupported_function": (lambda u, v: np.prod(u) * np.prod(v), 2, "not supported"),
    "vector_return": (lambda u, v: u * v, 3, "one scalar"),
    "tuple_return": (lambda u, v: (u[0], v[0]), 1, "one scalar"),
    "asymmetric": (lambda u, v: u[0] - v[0], 1, "not symmetric"),
    "asymmetric_scaled": (lambda u, v: np.exp(-(u[0] - 2.0 * v[0]) ** 2), 1, "not symmetric"),
    "too_many_instructions": (lambda u, v: _deep(u[0] * v[0]), 1, "at most 64"),
    "too_many_constants": (lambda u, v: sum((k + 1.5) * (u[0] * v[0]) ** 2 for k in range(33)), 1, "at most"),
    "non_finite_constant": (lambda u, v: u[0] * v[0] * float("inf"), 1, "not finite"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_the_tracer_refuses(B, case):
    f, d, word = BAD[case]
    with pytest.raises(ValueError) as e:
        B.DeviceKernel(f, d)
    assert "DeviceKernel" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("d", [0, 17, 40])
def test_x_dim_outside_1_to_16_is_refused(B, d):
    with pytest.raises(ValueError) as e:
        B.DeviceKernel(lambda u, v: (u * v).sum(), d)
    assert "1 to 16" in str(e.value)


def test_a_kernel_that_passes_through_zero_at_a_test_pair_is_not_called_asymmetric(B):
    """f(u, v) = u0 + v0 + u1 + v1 + … − c with c = its value at the self-check's first pair: f is 0 (or an ulp of the sums) there, and f(v, u)
    adds the same terms in another order.  The difference is ulps of the sums, far above 16 ulp of the tiny result and far below
    16 ulp of the kernel's size over the test pairs: symmetric.  u − v stays refused (test_the_tracer_refuses)."""
    d = 5
    rng = np.random.default_rng(0)                           # the pairs trace_kernel checks at
    U, V = rng.standard_normal((d, 8)), rng.standard_normal((d, 8))
    def zipped(u, v):                                        # ((u0 + v0) + u1) + v1 ...: swapping u and v re-associates the sum
        acc = u[0] + v[0]
        for k in range(1, d):
            acc = (acc + u[k]) + v[k]
        return acc
    c = float(zipped(U[:, 0], V[:, 0]))
    f = lambda u, v: zipped(u, v) - c                        # noqa: E731
    prog = B.DeviceKernel(f, d).program
    a, b = prog.eval(U, V), prog.eval(V, U)
    assert a[0] == 0.0 and np.abs(a).max() > 0.5
    assert np.any(a != b), "the pairs no longer tell the two orders apart: pick another d"
    print(f"[kern-host] zero crossing: f(u,v) = {a[0]!r}, f(v,u) = {b[0]!r}, max|f(u,v) - f(v,u)| {np.abs(a - b).max():.3e}")


def test_the_trace_sees_what_the_closure_hides(B):
    """A closure that answers the symbolic call and the numeric call differently fails the self-check against the closure."""
    def sly(u, v):
        return (u * v).sum() if isinstance(u, np.ndarray) else (u * v).sum() + 1.0
    with pytest.raises(ValueError) as e:
        B.DeviceKernel(sly, 2)
    assert "disagrees with the closure" in str(e.value)


def test_kern_create_rejects_bad_programs(api):
    lib = api.load_library()

    def create(d, consts, code, out_id):
        consts = np.asarray(consts, dtype=np.float64)
        code = np.ascontiguousarray(np.asarray(code, dtype=np.intc).reshape(-1, 3))
        h = C.c_void_p()
        rc = lib.boss_kern_create(d, consts.shape[0], api._dp(consts) if consts.size else None, code.shape[0],
                                  code.ctypes.data_as(C.POINTER(C.c_int)) if code.size else None, out_id, C.byref(h))
        if rc == 0:
            lib.boss_kern_free(h)
        return rc, lib.boss_last_error().decode()
    MUL, NEG = api.FIT_OP["MUL"], api.FIT_OP["NEG"]
    assert create(1, [], [(MUL, 0, 1)], 2)[0] == api.BOSS_OK                   # u[0] * v[0]
    for d in (0, 17, -3):
        rc, msg = create(d, [], [], 0)
        assert rc == api.BOSS_E_INVALID and "1 to 16" in msg
    bad = [
        (1, [], [(MUL, 0, 2)], 2, "earlier"),                                  # self reference
        (1, [], [(MUL, 0, 3)], 2, "earlier"),                                  # forward reference
        (1, [], [(99, 0, 1)], 2, "opcode"),
        (1, [], [(NEG, 0, 1)], 2, "unary"),
        (1, [], [(MUL, 0, -1)], 2, "operand b"),
        (1, [float("nan")], [], 0, "not finite"),
        (1, [], [(MUL, 0, 1)], 3, "out_id"),
        (1, [], [(MUL, 0, 1)], -1, "out_id"),
        (1, [1.0] * 33, [], 0, "32 constants"),
        (1, [], [(MUL, 0, 1)] * 65, 2, "64 instructions"),
        (2, [], [(MUL, 0, 4)], 4, "earlier"),                                  # 2·d = 4 inputs: id 4 is the instruction itself
    ]
    for d, consts, code, out_id, word in bad:
        rc, msg = create(d, consts, code, out_id)
        assert rc == api.BOSS_E_INVALID and word in msg, (d, code, msg)
    assert lib.boss_kern_create(1, 0, None, 0, None, 0, None) == api.BOSS_E_INVALID
    assert lib.boss_kern_eval_host(None, 1, None, None, None) == api.BOSS_E_INVALID


def test_kgp_create_rejects_bad_arguments(B, api):
    lib = api.load_library()
    prog = B.DeviceKernel(cases.expo, 2).program
    X, y = np.asfortranarray(np.zeros((2, 3))), np.zeros(3)
    h = C.c_void_p()
    calls = [
        (0, 2, 3, api._dp(X), api._dp(y), None, None, "kern is NULL"),
        (0, 3, 3, api._dp(X), api._dp(y), None, prog._h, "x_dim = 2"),
        (0, 2, 0, api._dp(X), api._dp(y), None, prog._h, "N >= 1"),
        (0, 2, 3, None, api._dp(y), None, prog._h, "non-NULL"),
        (0, 2, 3, api._dp(X), None, None, prog._h, "non-NULL"),
        (0, 2, 46081, api._dp(X), api._dp(y), None, prog._h, "46080"),
    ]
    for dev, d, N, Xp, yp, disc, kern, word in calls:
        rc = lib.boss_kgp_create(dev, d, N, Xp, yp, disc, kern, C.byref(h))
        assert rc == api.BOSS_E_INVALID and word in lib.boss_last_error().decode(), (d, N, lib.boss_last_error().decode())
        assert not h.value
    assert lib.boss_kgp_create(0, 2, 3, api._dp(X), api._dp(y), None, prog._h, None) == api.BOSS_E_INVALID
    with pytest.raises(TypeError):
        api.KernelGP(X, y, "matern52")


def test_models_that_take_no_device_kernel_say_so(B):
    dk = B.DeviceKernel(cases.expo, 2)
    pri = dict(lengthscale_priors=[B.MvLogNormal([0., 0.], [1., 1.])], amplitude_priors=[B.LogNormal()], noise_std_priors=[B.Dirac(0.1)])
    with pytest.raises(NotImplementedError, match="DeviceKernel"):
        B.HipGradientGaussianProcess(grad_noise_std_priors=[B.Dirac(0.1)], kernel=dk, **pri)
    with pytest.raises(NotImplementedError, match="DeviceKernel"):
        B.HipParametrizedGP([1.0, 1.0], kernel=dk)           # the latent models of a HipNonstationaryGP
    model = B.HipGaussianProcess(kernel=dk, **pri)
    with pytest.raises(NotImplementedError, match="DeviceKernel"):
        B.HipTransformedModel(model)
    # make_discrete keeps the kernel; a string kernel stays a string
    assert model.make_discrete([True, False]).kernel is dk
    assert B.HipGaussianProcess(**pri).kernel == "matern52"
