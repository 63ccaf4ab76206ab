"""Acquisition programs on the host (no GPU): tracing of closures into api.AcqProgram, boss_acqp_create's validation, the two new
opcodes through the library's interpreter (boss_acqp_eval_host — the function the kernels call) against 50-digit values, the
branch-free EI × feasibility spelling pinned on the fixture of tests/test_acq_tails_host.py, and the plugin level's dispatch."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acq_tails_cases as T  # noqa: E402


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd
    return boss_jl_amd


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def cases(B):
    import acq_program_cases
    return acq_program_cases


def moments(P, Q, n, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((P, n)), rng.uniform(0.05, 2.0, (P, n)), rng.standard_normal(Q)


# ------------------------------------------------------------------------------------------ 1. tracing
@pytest.mark.parametrize("name", ["ucb", "ucb1", "pi", "pi1", "max_variance", "clamp", "long_minmax", "ei_fp1", "ei_fp2", "ei_fp3"])
def test_traced_program_matches_closure_and_its_derivative(cases, name):
    f, P, Q = cases.CLOSURES[name]
    prog = cases.programs()[name]
    mu, var, q = moments(P, Q, 100)
    want = np.array([float(f(mu[:, k], var[:, k], q)) for k in range(100)])
    got = prog.eval(prog.stack(mu, var, q))
    assert np.all(np.abs(got - want) <= 1e-13 * np.maximum(1.0, np.abs(want)))
    a, dm, dv = prog.eval_host(mu, var, q, want_grad=True)
    assert np.all(np.abs(a - got) <= 1e-13 * np.maximum(1.0, np.abs(got)))
    g = prog.grad(prog.stack(mu, var, q))
    scale = max(np.abs(g).max(), 1.0)
    assert np.all(np.abs(dm - g[:P]) <= 1e-12 * scale) and np.all(np.abs(dv - g[P:2 * P]) <= 1e-12 * scale)
    # and the reverse sweep against central differences of the closure
    h = 1e-6
    for p in range(P):
        e = np.zeros((P, 1))
        e[p] = h
        dmu = (prog.eval(prog.stack(mu + e, var, q)) - prog.eval(prog.stack(mu - e, var, q))) / (2 * h)
        dva = (prog.eval(prog.stack(mu, var + e, q)) - prog.eval(prog.stack(mu, var - e, q))) / (2 * h)
        smooth = name not in ("clamp", "long_minmax")        # (a difference across a MIN / MAX kink is not the one-sided derivative)
        if smooth:
            assert np.all(np.abs(dmu - dm[p]) <= 1e-6 * scale) and np.all(np.abs(dva - dv[p]) <= 1e-6 * scale), (name, p)


def test_the_closures_reach_every_workgroup_shape(cases):
    """The launch rule of the two kernels on the traced programs: each runs with 1, 2, 3 and 4 waves somewhere (the device tests pick
    their programs by this; a closure that changes size cannot lose a shape silently)."""
    for grad in (False, True):
        seen = {cases.waves(p, grad) for p in cases.programs().values()}
        assert seen == {1, 2, 3, 4}, (grad, {n: cases.waves(p, grad) for n, p in cases.programs().items()})


def _sin_chain(x, n):
    for _ in range(n):
        x = np.sin(x)
    return x


def test_untraceable_closures_raise_value_errors(B):
    D = B.DeviceAcquisition
    with pytest.raises(ValueError, match="data-dependent control flow"):
        D(lambda mu, var, q: mu[0] if mu[0] > 0 else var[0], 1)
    with pytest.raises(ValueError, match="math"):
        D(lambda mu, var, q: math.sin(mu[0]), 1)
    with pytest.raises(ValueError, match="1 to 8 outputs"):
        D(lambda mu, var, q: mu.sum(), 9)
    with pytest.raises(ValueError, match="0 to 16 runtime scalars"):
        D(lambda mu, var, q: mu.sum(), 1, n_params=17, params=lambda p: np.zeros(17))
    with pytest.raises(ValueError, match="at most 32"):
        D(lambda mu, var, q: sum(mu[0] * (1.5 + k) for k in range(33)), 1)
    with pytest.raises(ValueError, match="at most 64"):
        D(lambda mu, var, q: _sin_chain(mu[0], 65), 1)
    with pytest.raises(ValueError, match="must return one scalar"):
        D(lambda mu, var, q: [mu[0], var[0]], 1)
    with pytest.raises(ValueError, match="must return one scalar"):
        D(lambda mu, var, q: mu * 2.0, 2)
    with pytest.raises(ValueError, match="needs params"):
        D(lambda mu, var, q: mu[0] + q[0], 1, n_params=1)
    with pytest.raises(ValueError, match="not supported"):
        D(lambda mu, var, q: np.arctan(mu[0]), 1)


def test_normal_functions_trace_only_in_an_acquisition(B, api):
    from scipy.special import ndtr
    p = B.DeviceAcquisition(lambda mu, var, q: ndtr(mu[0]) + B.normcdf(var[0]) * B.normpdf(mu[0]), 1).program
    assert sorted(int(op) for op in p.code[:, 0] if op >= 16) == [16, 16, 17]
    assert api.ACQ_OPS == api.FIT_OPS + ("NORMCDF", "NORMPDF") and len(api.FIT_OPS) == 16 and api.FIT_OP["MAX"] == 15
    z = np.array([-3.0, 0.0, 0.5])
    assert np.array_equal(B.normcdf(z), 0.5 * __import__("scipy.special").special.erfc(-z * 0.7071067811865476))
    assert np.array_equal(B.normpdf(z), np.exp(-0.5 * z * z) * 0.3989422804014327) and B.normcdf(0.0) == 0.5
    for f in (B.normcdf, B.normpdf, ndtr):
        with pytest.raises(ValueError, match="not supported in a device fitness"):
            B.DeviceFitness(lambda y: f(y[0]), 1)
        with pytest.raises(ValueError, match="not supported in a device mean"):
            B.DeviceMean(lambda x, th: [f(x[0]) * th[0]], 1, 1, 1)
        with pytest.raises(ValueError, match="not supported in a device kernel"):
            B.DeviceKernel(lambda u, v: f(u[0] - v[0]), 1)


# ------------------------------------------------------------------------------------------ 2. boss_acqp_create
def _create(api, name, args):
    h = C.c_void_p()
    rc = getattr(api.load_library(), name)(*args, C.byref(h))
    msg = api.load_library().boss_last_error().decode()
    if rc == 0:
        getattr(api.load_library(), name.replace("_create", "_free"))(h)
    return rc, msg


def _prog_args(consts, code, out_id):
    consts = np.asarray(consts, dtype=np.float64)
    code = np.ascontiguousarray(np.asarray(code, dtype=np.intc).reshape(-1, 3))
    return (len(consts), consts.ctypes.data_as(C.POINTER(C.c_double)) if len(consts) else None, code.shape[0],
            code.ctypes.data_as(C.POINTER(C.c_int)) if code.shape[0] else None, out_id), (consts, code)


@pytest.mark.parametrize("what, P, Q, consts, code, out_id", [
    ("1 to 8 outputs", 0, 0, [], [], 0),
    ("1 to 8 outputs", 9, 0, [], [], 0),
    ("0 to 16 runtime scalars", 1, 17, [], [], 0),
    ("0 to 16 runtime scalars", 1, -1, [], [], 0),
    ("at most 32 constants", 1, 0, [1.0] * 33, [], 0),
    ("at most 64 instructions", 1, 0, [], [[0, 0, 1]] * 65, 0),
    ("not finite", 1, 0, [np.inf], [], 0),
    ("unknown opcode 18", 1, 0, [], [[18, 0, -1]], 2),
    ("unknown opcode -1", 1, 0, [], [[-1, 0, -1]], 2),
    ("operand a must be an earlier value id", 1, 0, [], [[4, 2, -1]], 2),
    ("operand a must be an earlier value id", 1, 1, [], [[4, 3, -1]], 3),
    ("operand b must be an earlier value id", 1, 0, [], [[0, 0, 2]], 2),
    ("a unary operation takes b = -1", 1, 0, [], [[16, 0, 1]], 2),
    ("a unary operation takes b = -1", 1, 0, [], [[17, 0, 0]], 2),
    ("out_id is not a value id", 1, 0, [], [[16, 0, -1]], 3),
])
def test_acqp_create_refuses(api, what, P, Q, consts, code, out_id):
    args, keep = _prog_args(consts, code, out_id)
    rc, msg = _create(api, "boss_acqp_create", (P, Q) + args)
    assert rc == api.BOSS_E_INVALID and what in msg, (rc, msg)


def test_acqp_create_accepts_the_new_opcodes_and_fit_create_does_not(api):
    for op in (16, 17):
        args, keep = _prog_args([], [[op, 0, -1]], 2)
        assert _create(api, "boss_acqp_create", (1, 0) + args)[0] == api.BOSS_OK
        rc, msg = _create(api, "boss_fit_create", (2,) + args)
        assert rc == api.BOSS_E_INVALID and f"unknown opcode {op}" in msg
    args, keep = _prog_args([], [], 1)                       # (a program that is one of its inputs: σ² itself)
    assert _create(api, "boss_acqp_create", (1, 0) + args)[0] == api.BOSS_OK


# ------------------------------------------------------------------------------------------ 3. the new opcodes alone
def _unary(api, op, z):
    p = api.AcqProgram(1, 0, [], [[api.ACQ_OP[op], 0, -1]], 2)
    a, dm, _ = p.eval_host(np.array([[z]]), np.array([[1.0]]), None, want_grad=True)
    return float(a[0]), float(dm[0, 0])


def test_normcdf_and_normpdf_at_zero(api):
    assert _unary(api, "NORMCDF", 0.0) == (0.5, 0.3989422804014327)
    v, d = _unary(api, "NORMPDF", 0.0)
    assert v == 0.3989422804014327 and d == 0.0
    for z in (-2.5, 0.75, 3.0):
        v, d = _unary(api, "NORMPDF", z)
        assert d == -z * v


@pytest.mark.parametrize("z", [-30.0, -8.0, -1.0, 0.5, 6.0])
def test_new_opcodes_against_fifty_digits(api, z):
    """Relative bar (8 + 2z²)·2⁻⁵²: the rounding of the scaled argument x = z/√2 moves erfc by 2x² = z² relative (d log erfc(x) /
    d log x ≈ −2x² in the tail), exp(−z²/2) moves by z²/2 from the rounding of its argument and again from the rounded product
    0.5·z·z; a few ulp for the library function and the final scaling."""
    import mpmath as mp
    from oracle import mp_oracle as MP
    mp.mp.dps = 50
    bar = (8 + 2 * z * z) * 2.0 ** -52
    Phi, phi = MP._ncdf(mp.mpf(z)), MP._npdf(mp.mpf(z))
    v, d = _unary(api, "NORMCDF", z)
    r_v, r_d = float(abs(mp.mpf(v) - Phi) / Phi), float(abs(mp.mpf(d) - phi) / phi)
    w, e = _unary(api, "NORMPDF", z)
    r_w, r_e = float(abs(mp.mpf(w) - phi) / phi), float(abs(mp.mpf(e) + z * phi) / abs(z * phi))
    print(f"z {z}: relative errors Φ {r_v:.3g} Φ' {r_d:.3g} φ {r_w:.3g} φ' {r_e:.3g} against the bar {bar:.3g}")
    assert max(r_v, r_d, r_w, r_e) <= bar


# ------------------------------------------------------------------------------------------ 4. fixture pins
def test_the_rule_selects_enough_groups(cases):
    vg = cases.value_groups()
    assert len(vg) >= 24 and sum(g["M"] for g in vg) >= 2000, [g["name"] for g in vg]
    assert {g["S"] for g in vg} == {1, 3} and {g["P"] for g in vg} == {1, 2, 3}
    assert any(g["best"] is None for g in vg) and any(g["y_max"] is None for g in vg)
    assert {"g-tail-d1", "g-tail-d3"} <= set(cases.GRAD_GROUPS)


def test_numpy_restatement_stays_within_a_quarter_of_the_bar(cases):
    """The spelling itself, in numpy: what the fixture's truths say about it before any interpreter or device is asked.  Gradient
    groups beyond the two tail groups are on the list exactly when this restatement stays within device_C/4 on them."""
    hdr = T.load()["header"]
    worst = 0.0
    for g in cases.value_groups():
        r = T.ratio(cases.group_numpy(g), g["truth"], g["cond"])
        worst = max(worst, r)
        assert r <= hdr["device_C"]["value"] / 4, (g["name"], r)
    print(f"numpy restatement, values: worst err/(u·cond) {worst:.3g} over {len(cases.value_groups())} groups")
    listed = {}
    for g in cases.grad_candidates():
        val, grad = cases.group_numpy(g, want_grad=True)
        r = max(T.ratio(grad, g["gtruth"], g["gcond"]), T.ratio(val, g["truth"], g["cond"]))
        print(f"numpy reverse sweep, {g['name']}: err/(u·cond) {r:.3g}")
        if r <= hdr["device_C"]["grad"] / 4:
            listed[g["name"]] = r
    assert set(listed) == set(cases.GRAD_GROUPS), (listed, cases.GRAD_GROUPS)
    for n, r in listed.items():
        assert abs(r - cases.GRAD_GROUPS[n]) <= 0.5, (n, r, cases.GRAD_GROUPS[n])   # (the recorded ratios; libm may move a digit)


def interpreter_on_group(cases, g, want_grad=False):
    """The C interpreter on a fixture group, folded as the kernels fold: samples in ascending order, 1/S once."""
    prog, q = cases.group_program(g)
    if want_grad:
        a, dm, dv = prog.eval_host(g["mu"][0], g["var"][0], q, want_grad=True)
        return a, cases.fold(dm, dv, g["var"][0], g["dmu"], g["dvar"])
    acc = None
    for s in range(g["S"]):
        a = prog.eval_host(g["mu"][s], g["var"][s], q)
        acc = a if acc is None else acc + a
    return acc * (1.0 / g["S"]) if g["S"] > 1 else acc


def test_interpreter_values_on_the_fixture(cases):
    C_ = T.load()["header"]["device_C"]["value"]
    worst = 0.0
    for g in cases.value_groups():
        got = interpreter_on_group(cases, g)
        bad = T.misses(got, g["truth"], g["cond"], C_)
        worst = max(worst, T.ratio(got, g["truth"], g["cond"]))
        assert not bad.any(), (g["name"], np.flatnonzero(bad)[:5], T.ratio(got, g["truth"], g["cond"]))
    print(f"C interpreter, values: worst err/(u·cond) {worst:.3g} against C = {C_}")


def test_interpreter_gradients_on_the_fixture(cases):
    C_ = T.load()["header"]["device_C"]["grad"]
    for g in cases.grad_groups():
        val, grad = interpreter_on_group(cases, g, want_grad=True)
        print(f"C interpreter, {g['name']}: value {T.ratio(val, g['truth'], g['cond']):.3g} gradient {T.ratio(grad, g['gtruth'], g['gcond']):.3g} "
              f"against C = {C_}")
        assert not T.misses(val, g["truth"], g["cond"], T.load()["header"]["device_C"]["value"]).any(), g["name"]
        assert not T.misses(grad, g["gtruth"], g["gcond"], C_).any(), g["name"]


# ------------------------------------------------------------------------------------------ 5. plugin level without a device
def _gp(B, P=1):
    return B.HipGaussianProcess(lengthscale_priors=[None] * P, amplitude_priors=[None] * P, noise_std_priors=[None] * P)


def _problem(B, acq, model=None, P=1):
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (2, 12))
    Y = np.vstack([np.sin(3 * X[0]) + X[1] + 0.1 * p for p in range(P)])
    dom = B.Domain(bounds=(np.zeros(2), np.ones(2)))
    return B.BossProblem(f=None, domain=dom, acquisition=acq, model=model if model is not None else _gp(B, P), data=B.ExperimentData(X, Y))


def test_problem_accepts_a_device_acquisition_and_modes_refuse_it(B):
    acq = B.UpperConfidenceBound(B.LinFitness([1.0]), 2.0)
    prob = _problem(B, acq)
    assert prob.acquisition is acq and acq.fitness.coefs == [1.0] and acq.outside == -np.inf and acq.cons_safe
    am = B.HipBatchAM(points=np.random.default_rng(1).uniform(0, 1, (2, 5)), devices=[0])
    with pytest.raises(NotImplementedError, match="DeviceAcquisition"):
        am.maximize_acquisition(prob)
    warped = B.HipTransformedModel(_gp(B))
    for m in (B.HipBatchAM(points=np.zeros((2, 3))), B.HipGradientAM(x_prior=lambda rng: rng.uniform(0, 1, 2), multistart=2, iters=1)):
        with pytest.raises(NotImplementedError, match="DeviceAcquisition"):
            m.maximize_acquisition(_problem(B, acq, warped))


def test_params_is_called_once_per_maximisation(B, monkeypatch):
    from boss_jl_amd import maximizer
    calls = []

    def params(problem):
        calls.append(problem.data.Y.shape[1])
        return [np.inf]
    acq = B.DeviceAcquisition(lambda mu, var, q: mu[0] - np.minimum(q[0], var[0]), 1, n_params=1, params=params)
    prob = _problem(B, acq)
    seen = []
    monkeypatch.setattr(maximizer, "posteriors_of", lambda *a, **k: [])
    monkeypatch.setattr(maximizer, "_program_values", lambda problem, posts, Xs, cand, q: (seen.append(q), (np.zeros(Xs.shape[1]), 0, 0.0))[1])
    B.HipBatchAM(points=np.zeros((2, 3)), fused=True).maximize_acquisition(prob)
    assert calls == [12] and np.array_equal(seen[0], [np.inf])
    # the ascent: one call however many iterations evaluate the acquisition
    monkeypatch.setattr(maximizer.HipGradientAM, "_program_value_and_grad",
                        lambda self, problem, posts, X: (seen.append(self.__dict__["_acq_q"]), (np.arange(X.shape[1], dtype=float), np.ones(X.shape)))[1])
    B.HipGradientAM(x_prior=lambda rng: rng.uniform(0, 1, 2), multistart=4, iters=3, seed=0).maximize_acquisition(prob)
    assert calls == [12, 12] and len(seen) == 1 + 4 and all(np.array_equal(s, [np.inf]) for s in seen)
    with pytest.raises(ValueError, match="returned 2 values"):
        B.DeviceAcquisition(lambda mu, var, q: mu[0] + q[0], 1, n_params=1, params=lambda p: [1.0, 2.0]).scalars(prob)
    with pytest.raises(ValueError, match="y_dim = 1"):
        acq.scalars(_problem(B, acq, P=2))
