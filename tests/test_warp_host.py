"""Warps without a device: the handle (boss_warp_create), the host twins of the two stages (boss_warp_apply_host,
boss_warp_moments_host: the functions the kernels call) against the 50-digit truths of tests/golden/warp.json, the identities and
refusals of the C ABI, the traced transforms, and HipTransformedModel's host-side semantics.

Stage bounds: values 1e-13 relative, gradients 1e-12 relative, element by element.  Chain bars: tests/warp_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_cases as W  # noqa: E402

NAMES = list(W.CASES)


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def fx():
    return W.load()


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


def test_the_fixture_covers_the_shapes_and_transforms(fx):
    assert {W.CASES[n][:5] for n in NAMES} == {(2, 3, 12, 6, 1), (3, 2, 12, 6, 2), (2, 2, 40, 6, 2)}
    assert fx["dps"] == 50 and set(fx["cases"]) == set(NAMES)
    for n in NAMES:
        du, dm, N, M, P = W.CASES[n][:5]
        c = fx["cases"][n]
        assert c["X_"].shape == (dm, M) and c["J"].shape == (M, dm, du) and c["mu"].shape == (P, M) and c["dvar"].shape == (P, du, M)
        nz = np.abs(c["J"][c["J"] != 0])
        assert nz.min() >= 1e-3 and nz.max() <= 1e3
        assert np.all(c["var_"] > 1e-6)                      # no candidate near the variance clip: one code path


@pytest.mark.parametrize("name", NAMES)
def test_input_warp_host_twin_against_50_digits(B, fx, name):
    c = fx["cases"][name]
    Xs = W.data(name)[1]
    w = W.warp_program(B, name)
    X_, J = w.apply_host(Xs, True)
    nz = c["J"] != 0
    ev, eg = _rel(X_, c["X_"]), _rel(J[nz], c["J"][nz])
    print(f"[warp-host] {name}: x_ rel err {ev:.3e} (1e-13), J rel err {eg:.3e} (1e-12)")
    assert ev <= 1e-13 and eg <= 1e-12
    assert np.all(J[~nz] == 0.0)                             # structural zeros of the Jacobian are exact
    assert np.array_equal(w.apply_host(Xs, False)[0], X_)    # without the sweep: the same values


@pytest.mark.parametrize("name", NAMES)
def test_moments_host_twin_against_50_digits(B, fx, name):
    """The stage on the fixture's rounded model-space arrays against the same stage at 50 digits."""
    c = fx["cases"][name]
    w = W.warp_program(B, name)
    mu, var, dmu, dvar = w.moments_host(c["mu_"], c["var_"], c["dmu_"], c["dvar_"], c["J"])
    errs = {k: _rel(g, c["fold_" + k]) for k, g in (("mu", mu), ("var", var), ("dmu", dmu), ("dvar", dvar))}
    print(f"[warp-host] {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert errs["mu"] <= 1e-13 and errs["var"] <= 1e-13 and errs["dmu"] <= 1e-12 and errs["dvar"] <= 1e-12
    mu2, var2 = w.moments_host(c["mu_"], c["var_"])          # values alone: the same bits
    assert np.array_equal(mu2, mu) and np.array_equal(var2, var)


@pytest.mark.parametrize("name", NAMES)
def test_chain_on_the_host_twin_within_the_scaled_regimes_bars(B, fx, name):
    """50-digit posterior moments and moment gradients (rounded) -> fold -> user space, against the truth of the WHOLE chain."""
    c = fx["cases"][name]
    N = W.CASES[name][2]
    w = W.warp_program(B, name)
    mu, var, dmu, dvar = w.moments_host(c["mu_"], c["var_"], c["dmu_"], c["dvar_"], c["J"])
    vb, gb = W.chain_bars(c, N)
    ev = max(np.abs(mu - c["mu"]).max(), np.abs(var - c["var"]).max())
    eg = max(np.abs(dmu - c["dmu"]).max(), np.abs(dvar - c["dvar"]).max())
    print(f"[warp-host] {name}: chain value err/bar {ev / vb:.3e}, gradient err/bar {eg / gb:.3e} (L {c['L']:.3g})")
    assert ev <= vb and eg <= gb


def test_teeth_a_transposed_jacobian_or_a_wrong_sigma_gradient_misses_a_bar(B, fx):
    """Deliberately wrong arrays into the host twin's stages: J transposed (where it is square), and ∇var_ doubled, which is what
    ∇σ_ = ∇var_/σ_ in place of ∇var_/(2σ_) would compute.  Each must miss the chain's gradient bar in at least one case."""
    missed_t = missed_s = False
    for name in NAMES:
        c = fx["cases"][name]
        du, dm, N = W.CASES[name][0], W.CASES[name][1], W.CASES[name][2]
        w = W.warp_program(B, name)
        _, gb = W.chain_bars(c, N)
        err = lambda r: max(np.abs(r[2] - c["dmu"]).max(), np.abs(r[3] - c["dvar"]).max())          # noqa: E731
        if du == dm:
            missed_t |= err(w.moments_host(c["mu_"], c["var_"], c["dmu_"], c["dvar_"], c["J"].transpose(0, 2, 1))) > gb
        missed_s |= err(w.moments_host(c["mu_"], c["var_"], c["dmu_"], 2.0 * c["dvar_"], c["J"])) > gb
    assert missed_t and missed_s


# ---------------------------------------------------------------------------------------------- identities
def _rand_moments(rng, S, P, M, dm):
    return (rng.uniform(1.0, 2.0, (S, P, M)), rng.uniform(0.05, 0.4, (S, P, M)), rng.standard_normal((S, P, dm, M)),
            rng.standard_normal((S, P, dm, M)))


def test_clipped_and_zero_variances_give_no_sigma_gradient(B):
    w = W.warp_program(B, "logw-affine")
    rng = np.random.default_rng(3)
    mu_, var_, dmu_, dvar_ = _rand_moments(rng, 2, 2, 5, 2)
    J = rng.uniform(0.5, 2.0, (5, 2, 2))
    var_[0, 0, 1], var_[1, 1, 3] = 0.0, -5e-9                # zero, and inside the clip
    mu, var, dmu, dvar = w.moments_host(mu_, var_, dmu_, dvar_, J)
    zero = dvar_.copy()
    zero[0, 0, :, 1] = 0.0
    zero[1, 1, :, 3] = 0.0
    varc = var_.copy()
    varc[1, 1, 3] = 0.0
    ref = w.moments_host(mu_, varc, dmu_, zero, J)
    for a, b in zip((mu, var, dmu, dvar), ref):
        assert np.array_equal(a, b)
    assert var[0, 0, 1] == 0.0 and var[1, 1, 3] == 0.0 and np.all(dvar[0, 0, :, 1] == 0.0) and np.all(dvar[1, 1, :, 3] == 0.0)
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))


def test_a_variance_below_the_clip_follows_the_callers_convention(B, api):
    w = W.warp_program(B, "kuma-mix")
    rng = np.random.default_rng(4)
    mu_, var_, dmu_, dvar_ = _rand_moments(rng, 2, 2, 7, 2)
    J = rng.uniform(0.5, 2.0, (7, 2, 3))
    clean = w.moments_host(mu_, var_, dmu_, dvar_, J)
    var_[1, 0, 4] = -1e-3
    var_[1, 1, 2] = -2e-3                                    # later in memory, smaller candidate index: memory order decides
    with pytest.raises(api.DomainError) as e:                # the prediction calls' convention
        w.moments_host(mu_, var_, dmu_, dvar_, J)
    assert e.value.code == api.BOSS_E_NEG_VAR and e.value.bad_index == 4
    mu, var, dmu, dvar = w.moments_host(mu_, var_, dmu_, dvar_, J, check=False)          # the acquisition calls' convention
    for j in (4, 2):
        assert np.array_equal(mu[1, :, j], mu_[1, :, j]) and np.array_equal(var[1, :, j], var_[1, :, j])      # passed through: still below the clip
        assert np.all(dmu[1, :, :, j] == 0.0) and np.all(dvar[1, :, :, j] == 0.0)
    keep = np.ones((2, 7), bool)
    keep[1, 4] = keep[1, 2] = False
    for a, b in zip((mu, var), clean[:2]):
        assert np.array_equal(a.transpose(0, 2, 1)[keep], b.transpose(0, 2, 1)[keep])
    for a, b in zip((dmu, dvar), clean[2:]):
        assert np.array_equal(a.transpose(0, 3, 1, 2)[keep], b.transpose(0, 3, 1, 2)[keep])


def test_a_nan_at_one_candidate_leaves_its_neighbours_bits(B):
    w = W.warp_program(B, "feature-log")
    rng = np.random.default_rng(5)
    Xs = rng.uniform(0.3, 1.0, (2, 9))
    clean = w.apply_host(Xs, True)
    Xb = Xs.copy()
    Xb[1, 3] = np.nan
    bad = w.apply_host(Xb, True)
    ok = np.arange(9) != 3
    assert np.isnan(bad[0][2, 3]) and np.array_equal(bad[0][:, ok], clean[0][:, ok]) and np.array_equal(bad[1][ok], clean[1][ok])
    mu_, var_, dmu_, dvar_ = _rand_moments(rng, 1, 1, 9, 3)
    cm = w.moments_host(mu_, var_, dmu_, dvar_, clean[1])
    mu_[0, 0, 3] = -1.0                                      # log of a negative mean: NaN, as computed
    bm = w.moments_host(mu_, var_, dmu_, dvar_, clean[1])
    assert np.isnan(bm[0][0, 0, 3])
    for a, b in zip(bm, cm):
        assert np.array_equal(a[..., ok], b[..., ok])


def test_an_identity_output_program_passes_moments_through_bit_for_bit(B):
    w = W.warp_program(B, "kuma-mix", with_out=False)
    rng = np.random.default_rng(6)
    mu_, var_, dmu_, dvar_ = _rand_moments(rng, 3, 2, 6, 2)
    var_[2, 1, 5] = -3e-9                                    # inside the clip: passed through as it is
    J = rng.uniform(-2.0, 2.0, (6, 2, 3))
    mu, var, dmu, dvar = w.moments_host(mu_, var_, dmu_, dvar_, J)
    assert np.array_equal(mu, mu_) and np.array_equal(var, var_)
    for got, g_ in ((dmu, dmu_), (dvar, dvar_)):             # only J' is applied, summed in ascending k'
        want = np.zeros_like(got)
        for kk in range(2):
            want += J[:, kk, :].T[None, None] * g_[:, :, kk:kk + 1, :]
        assert np.array_equal(got, want)
    wo = W.warp_program(B, "kuma-mix", with_in=False)        # no input program: the gradients keep their dimension
    r = wo.moments_host(mu_, np.abs(var_), dmu_, dvar_, None, d_user=2)
    assert r[2].shape == (3, 2, 2, 6)


def test_a_sliced_transform_packed_as_a_joint_one_equals_the_scalar_closures(B):
    fw, bw = W.sliced_closures("logw-affine")
    t = B.DeviceSlicedOutputTransform(fw, bw)
    plain = B.SlicedOutputTransform(fw, bw)
    w = B.api.WarpProgram(None, 2, t.program)
    rng = np.random.default_rng(7)
    mu_, var_, dmu_, dvar_ = _rand_moments(rng, 1, 2, 8, 3)
    mu, var, dmu, dvar = w.moments_host(mu_, var_, dmu_, dvar_, None, d_user=3)
    m_ref, s_ref = plain.forward_cols(mu_[0], np.sqrt(var_[0]))
    assert np.array_equal(mu[0], m_ref) and np.array_equal(var[0], s_ref * s_ref)
    assert np.all(s_ref[1] < 0)                              # a negative std squares to the variance all the same
    # cross-derivatives are exact zeros: output p's gradients are a_p·∇mu_p and a_p²·∇var_p — nothing of the other output, and no rounding
    # beyond the products'
    for p, (a, _) in enumerate(W.AFFINE):
        assert np.array_equal(dmu[0, p], a * dmu_[0, p])
        sd = np.sqrt(var_[0, p])
        assert np.array_equal(dvar[0, p], 2.0 * (a * sd) * (a * (dvar_[0, p] / (2.0 * sd))))
    mu_b = mu_.copy()
    mu_b[0, 1] += 1.0                                        # moving output 1 leaves output 0's results untouched
    rb = w.moments_host(mu_b, var_, dmu_, dvar_, None, d_user=3)
    assert np.array_equal(rb[0][0, 0], mu[0, 0]) and np.array_equal(rb[2][0, 0], dmu[0, 0]) and np.array_equal(rb[3][0, 0], dvar[0, 0])


# ---------------------------------------------------------------------------------------------- refusals of the C ABI
def test_every_invalid_case_of_the_handle_fires(B, api):
    lib = api.load_library()
    ip = B.trace_mean(W.in_closure("feature-log"), 2, 0, 3)
    op1 = B.trace_mean(lambda z: [z[0], z[1]], 2, 0, 2)
    with_T = B.trace_mean(lambda x, th: [x[0] * th[0], x[1]], 2, 1, 2)
    wide = B.trace_mean(lambda x: [x.sum()], 17, 0, 1)
    h = C.c_void_p()

    def refused(a, P, b, word):
        assert lib.boss_warp_create(a, P, b, C.byref(h)) == api.BOSS_E_INVALID and not h
        assert word in lib.boss_last_error().decode(), lib.boss_last_error().decode()

    refused(None, 1, None, "needs an input program")
    refused(with_T._h, 2, None, "T must be 0")
    refused(None, 1, with_T._h, "T must be 0")
    refused(wide._h, 1, None, "x_dim <= 16")
    refused(None, 2, op1._h, "inputs, 2P = 4")               # wrong input count
    three = B.trace_mean(lambda z: [z[0], z[1], z[0]], 2, 0, 3)
    refused(None, 1, three._h, "outputs, 2P = 2")            # wrong output count
    refused(ip._h, 0, None, "1 to 16 outputs")
    refused(ip._h, 17, None, "1 to 16 outputs")
    refused(ip._h, 9, op1._h, "1 to 8 outputs")
    assert lib.boss_warp_create(ip._h, 1, op1._h, None) == api.BOSS_E_INVALID
    lib.boss_warp_free(None)
    w = api.WarpProgram(ip, 1, op1)
    ip.close()                                               # the warp owns its copies
    op1.close()
    X_, _ = w.apply_host(np.array([[0.5], [0.25]]))
    assert np.allclose(X_[:, 0], [0.5, 0.125, np.sin(0.25)], rtol=1e-15)


def test_stage_calls_refuse_bad_arguments_without_a_device(B, api):
    lib = api.load_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    w = W.warp_program(B, "feature-log")
    wo = W.warp_program(B, "feature-log", with_in=False)
    x, o = np.zeros(64), np.zeros(64)
    for fn, head in ((lib.boss_warp_apply_host, ()), (lib.boss_warp_apply, (0,))):
        assert fn(*head, None, 1, dp(x), dp(o), None) == api.BOSS_E_INVALID
        assert fn(*head, wo._h, 1, dp(x), dp(o), None) == api.BOSS_E_INVALID and "no input program" in lib.boss_last_error().decode()
        assert fn(*head, w._h, 0, dp(x), dp(o), None) == api.BOSS_E_INVALID
        assert fn(*head, w._h, 1, None, dp(o), None) == api.BOSS_E_INVALID
    for fn, head in ((lib.boss_warp_moments_host, ()), (lib.boss_warp_moments, (0,))):
        call = lambda wh, S, M, du, *ptrs: fn(*head, wh, S, M, du, *ptrs, None)      # noqa: E731
        full = [dp(x)] * 9
        assert call(None, 1, 1, 2, *full) == api.BOSS_E_INVALID
        assert call(w._h, 0, 1, 2, *full) == api.BOSS_E_INVALID
        assert call(w._h, 1, 1, 17, *full) == api.BOSS_E_INVALID
        assert call(w._h, 1, 1, 3, *full) == api.BOSS_E_INVALID and "input program takes 2" in lib.boss_last_error().decode()
        assert call(w._h, 1, 1, 2, dp(x), dp(x), dp(x), None, dp(x), dp(x), dp(x), dp(x), dp(x)) == api.BOSS_E_INVALID      # gradients partly given
        assert call(w._h, 1, 1, 2, dp(x), dp(x), dp(x), dp(x), None, dp(x), dp(x), dp(x), dp(x)) == api.BOSS_E_INVALID      # no J under an input program
        assert call(w._h, 1, 1, 2, dp(x), dp(x), None, None, dp(x), dp(x), dp(x), None, None) == api.BOSS_E_INVALID          # J without gradients
        assert call(wo._h, 1, 1, 2, *full) == api.BOSS_E_INVALID and "no input program" in lib.boss_last_error().decode()
        assert call(w._h, 1, 1, 2, None, dp(x), None, None, None, dp(x), dp(x), None, None) == api.BOSS_E_INVALID


def test_one_call_paths_refuse_bad_arguments_before_any_device_work(B, api):
    lib = api.load_library()
    w = W.warp_program(B, "feature-log")
    x = np.zeros(8)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.boss_warp_predict(None, 1, 1, None, 1, dp, None, dp, dp, None) == api.BOSS_E_INVALID
    assert lib.boss_warp_predict(w._h, 1, 1, None, 1, dp, None, dp, dp, None) == api.BOSS_E_INVALID
    arr = (C.c_void_p * 2)()
    assert lib.boss_warp_predict(w._h, 2, 1, arr, 1, dp, None, dp, dp, None) == api.BOSS_E_INVALID
    assert "created for 1 outputs" in lib.boss_last_error().decode()
    assert lib.boss_acq_ei_warp(w._h, 1, 1, arr, 1, dp, None, dp, None, 0, 0.0, None, dp, None, None) == api.BOSS_E_INVALID      # NULL handle
    assert lib.boss_acq_ei_grad_warp(w._h, 1, 1, arr, 1, dp, None, None, dp, None, 0, 0.0, None, None, dp) == api.BOSS_E_INVALID


# ---------------------------------------------------------------------------------------------- tracing
def test_tracing_refusals_and_the_backward_check(B):
    with pytest.raises(ValueError, match="DeviceInputTransform: the closure compares a traced value"):
        B.DeviceInputTransform(lambda x: [x[0] if x[0] > 0 else x[1]], 2, 1)
    with pytest.raises(ValueError, match="DeviceInputTransform: the closure returned 2 outputs, y_dim is 3"):
        B.DeviceInputTransform(lambda x: [x[0], x[1]], 2, 3)
    with pytest.raises(ValueError, match="DeviceInputTransform.*not supported in a device mean"):
        B.DeviceInputTransform(lambda x: [np.arctan(x[0])], 1, 1)
    with pytest.raises(ValueError, match="x_dim <= 16"):
        B.DeviceInputTransform(lambda x: [x.sum()], 17, 1)
    with pytest.raises(ValueError, match="DeviceInputTransform: the traced program disagrees with the closure"):
        calls = []
        B.DeviceInputTransform(lambda x: [x[0] * (1.0 if not calls.append(0) and len(calls) < 2 else 2.0)], 1, 1)
    with pytest.raises(ValueError, match="DeviceOutputTransform: y_dim = 9"):
        B.DeviceOutputTransform(lambda y, s: (y, s), lambda y: y, 9)
    with pytest.raises(ValueError, match="DeviceOutputTransform: the closure returned 3 outputs"):
        B.DeviceOutputTransform(lambda y, s: ([y[0], y[0]], [s[0]]), lambda y: y, 1)
    with pytest.raises(ValueError, match="DeviceOutputTransform: forward\\(backward\\(y\\)\\) does not return y"):
        B.DeviceOutputTransform(W.out_closure("feature-log"), lambda y: y, 1)
    with pytest.raises(ValueError, match="DeviceSlicedOutputTransform: forward\\(backward\\(y\\)\\) does not return y"):
        B.DeviceSlicedOutputTransform([lambda y, s: (2 * y, 2 * s)], [lambda y: y])
    with pytest.raises(ValueError, match="same length"):
        B.SlicedOutputTransform([lambda y, s: (y, s)], [])
    t = B.DeviceInputTransform(W.in_closure("feature-log"), 2, 3)
    assert np.array_equal(np.asarray(t(np.array([0.5, 0.25]))), [0.5, 0.125, np.sin(0.25)])          # calling it calls the closure
    o = B.DeviceOutputTransform(W.out_closure("kuma-mix"), W.back_mix, 2)
    assert (o.program.d, o.program.P, o.program.T) == (4, 4, 0)


# ---------------------------------------------------------------------------------------------- the Python layer on the library's CPU paths
class _StubBase:
    """What HipTransformedPosterior asks of a base posterior, on the host."""
    slices = []

    def mean_and_var(self, x):
        x = np.asarray(x, float)
        return np.stack([x.sum(0) + 2.0, 2.0 * x.sum(0) + 3.0]), np.stack([0.1 + x[0] ** 2, 0.2 + x[0] ** 2])

    def mean_and_cov(self, X):
        mu, var = self.mean_and_var(X)
        M = X.shape[1]
        cov = np.stack([np.full((M, M), 0.01) + np.diag(var[p] - 0.01) for p in range(2)], axis=2)
        return mu, cov

    def close(self):
        pass


def _gp(B, P=2, **kw):
    return B.HipGaussianProcess([B.MvLogNormal([0.0, 0.0], [1.0, 1.0])] * P, [B.LogNormal(0.0, 1.0)] * P, [B.LogNormal(-2.0, 1.0)] * P, **kw)


def test_transform_data_semantics_and_the_sliceable_table(B):
    base = _gp(B)
    it = B.InputTransform(W.in_closure("logw-affine"))
    fw, bw = W.sliced_closures("logw-affine")
    sl = B.SlicedOutputTransform(fw, bw)
    jt = B.JointOutputTransform(W.out_closure("kuma-mix"), W.back_mix)
    rng = np.random.default_rng(8)
    data = B.ExperimentData(rng.uniform(0.2, 1.0, (2, 5)), rng.standard_normal((2, 5)))
    m = B.HipTransformedModel(base, it, sl)
    td = m.transform_data(data)
    assert np.array_equal(td.X, np.stack([W.in_closure("logw-affine")(data.X[:, j]) for j in range(5)], axis=1))      # x forward, column by column
    assert np.allclose(td.X, np.stack([np.log(data.X[0] + 0.1), np.log(data.X[1] + 0.5 * data.X[0] + 0.1)]), rtol=1e-15)
    assert np.array_equal(td.Y, np.stack([(data.Y[i] - b) / a for i, (a, b) in enumerate(W.AFFINE)]))      # y backward, per output
    tj = B.HipTransformedModel(base, None, jt).transform_data(data)
    assert np.array_equal(tj.X, data.X)
    assert np.array_equal(tj.Y, np.stack([W.back_mix(data.Y[:, j]) for j in range(5)], axis=1))
    back = np.stack([np.asarray(W.out_closure("kuma-mix")(tj.Y[:, j], np.ones(2))[0]) for j in range(5)], axis=1)
    assert np.allclose(back, data.Y, rtol=1e-13, atol=1e-13)                             # forward(backward(y)) = y
    none = B.HipTransformedModel(base)
    assert none.transform_data(data) is data and none.warp is None
    # sliceable (transformed.jl:178-180): the base model's, and never under a joint output transform
    assert none.sliceable and m.sliceable and B.HipTransformedModel(base, it).sliceable
    assert not B.HipTransformedModel(base, None, jt).sliceable and not B.HipTransformedModel(base, it, jt).sliceable
    # a warp program exists only when EVERY given transform is a traced one
    dit = B.DeviceInputTransform(W.in_closure("logw-affine"), 2, 2)
    dsl = B.DeviceSlicedOutputTransform(fw, bw)
    assert B.HipTransformedModel(base, dit, dsl).warp is not None and B.HipTransformedModel(base, dit).warp is not None
    assert B.HipTransformedModel(base, dit, sl).warp is None and B.HipTransformedModel(base, it, dsl).warp is None
    assert B.HipTransformedModel(base, dit, dsl).sliceable
    # parameters are the base model's
    p = m.params_sampler()(np.random.default_rng(0))
    assert isinstance(p, B.HipGPParams) and m.params_loglike()(p) == base.params_loglike()(p)
    with pytest.raises(ValueError, match="slices"):
        B.HipTransformedModel(_gp(B, 1), None, sl)
    with pytest.raises(NotImplementedError, match="base"):
        B.HipTransformedModel(object())


def test_the_posterior_on_the_host_follows_the_reference(B):
    from boss_jl_amd.transformed import HipTransformedPosterior
    base = _gp(B)
    fw, bw = W.sliced_closures("logw-affine")
    it = B.InputTransform(W.in_closure("logw-affine"))
    stub = _StubBase()
    X = np.random.default_rng(9).uniform(0.2, 1.0, (2, 4))
    X_ = it.apply(X)
    mu_, var_ = stub.mean_and_var(X_)
    post = HipTransformedPosterior(B.HipTransformedModel(base, it, B.SlicedOutputTransform(fw, bw)), stub)
    mu, var = post.mean_and_var(X)
    assert np.array_equal(mu, np.stack([a * mu_[i] + b for i, (a, b) in enumerate(W.AFFINE)]))
    assert np.array_equal(var, np.stack([(a * np.sqrt(var_[i])) ** 2 for i, (a, _) in enumerate(W.AFFINE)]))
    m1, v1 = post.mean_and_var(X[:, 2])                                                # a vector: vectors of length P
    assert np.array_equal(m1, mu[:, 2]) and np.array_equal(v1, var[:, 2])
    assert np.array_equal(post.mean(X), mu) and np.array_equal(post.var(X), var) and np.array_equal(post.std(X), np.sqrt(var))
    m2, cov = post.mean_and_cov(X)                                                      # sliced: the diagonals are replaced, the rest stays
    _, cov_ = stub.mean_and_cov(X_)
    idx = np.arange(4)
    assert np.array_equal(m2, mu) and np.array_equal(cov[idx, idx, :].T, var)
    off = ~np.eye(4, dtype=bool)
    assert np.array_equal(cov[off], cov_[off])
    joint = HipTransformedPosterior(B.HipTransformedModel(base, it, B.JointOutputTransform(W.out_closure("kuma-mix"), W.back_mix)), stub)
    with pytest.raises(RuntimeError, match="Cannot compute covariance with joint output transform"):
        joint.mean_and_cov(X)
    mj, vj = joint.mean_and_var(X)
    want = [W.out_closure("kuma-mix")(mu_[:, k], np.sqrt(var_[:, k])) for k in range(4)]
    assert np.array_equal(mj, np.stack([np.asarray(w_[0]) for w_ in want], axis=1))
    assert np.array_equal(vj, np.stack([np.asarray(w_[1]) ** 2 for w_ in want], axis=1))
    only_in = HipTransformedPosterior(B.HipTransformedModel(base, it), stub)
    assert np.array_equal(only_in.mean_and_var(X)[0], mu_) and np.array_equal(only_in.mean_and_cov(X)[1], cov_)
    ident = HipTransformedPosterior(B.HipTransformedModel(base), stub)                  # None / None: the base model's results
    assert np.array_equal(ident.mean_and_var(X)[0], stub.mean_and_var(X)[0]) and np.array_equal(ident.mean_and_cov(X)[1], stub.mean_and_cov(X)[1])
    assert np.array_equal(B.average_mean([post, post], X), mu)
    with pytest.raises(NotImplementedError, match="plain closure has no derivative"):
        post.mean_and_var_grad(X)
    with pytest.raises(NotImplementedError, match="appending"):
        post.append(X[:, 0], np.zeros(2))


def test_maximizers_refuse_what_is_out_of_scope(B):
    base = _gp(B, 1)
    model = B.HipTransformedModel(base, B.InputTransform(lambda x: [np.log(x[0] + 0.1), x[1]]))
    dom = B.Domain(bounds=([0.2, 0.2], [1.0, 1.0]))
    rng = np.random.default_rng(10)
    data = B.ExperimentData(rng.uniform(0.2, 1.0, (2, 6)), rng.standard_normal((1, 6)))
    prob = B.BossProblem(f=None, model=model, data=data, domain=dom, acquisition=B.ExpectedImprovement(B.LinFitness([1.0])), y_max=[np.inf])
    pts = rng.uniform(0.2, 1.0, (2, 4))
    for am in (B.HipBatchAM(points=pts, shard="outputs"), B.HipBatchAM(points=pts, shard="samples"), B.HipBatchAM(points=pts, devices=[0])):
        with pytest.raises(NotImplementedError, match="HipTransformedModel"):
            am.maximize_acquisition(prob)
    with pytest.raises(NotImplementedError, match="HipTransformedModel"):
        B.HipSequentialBatchAM(B.HipBatchAM(points=pts), 2).maximize_acquisition(prob)
    from boss_jl_amd.transformed import HipTransformedPosterior, warped_acquisition_values, warped_value_and_grad
    posts = [HipTransformedPosterior(model, _StubBase())]
    with pytest.raises(NotImplementedError, match="plain closure has no derivative"):  # what a plain NonlinFitness gets from HipGradientAM
        B.HipGradientAM(x_prior=lambda r: r.uniform(0.2, 1.0, 2), multistart=2)._value_and_grad(prob, posts, pts)
    prob_n = B.BossProblem(f=None, model=model, data=data, domain=dom, acquisition=B.ExpectedImprovement(B.NonlinFitness(lambda y: y[0])), y_max=[np.inf])
    with pytest.raises(NotImplementedError, match="NonlinFitness"):
        warped_acquisition_values(prob_n, posts, pts)
    with pytest.raises(NotImplementedError, match="NonlinFitness"):
        warped_value_and_grad(prob_n, posts, pts)


def test_gradient_observations_reach_model_space_through_both_jacobians(B):
    """HipTransformedModel over a HipGradientGaussianProcess: with y_ = g(x_), x_ = w(x), y = a·y_ + b the user-space observations are
    ∂y/∂x = a·∇g·J; transform_data must hand the base model ∇g itself (dY_ = A⁻¹·dY·J⁻¹), and X_, Y_ as for any model."""
    fw, bw = W.sliced_closures("logw-affine")
    win = W.in_closure("logw-affine")
    base = B.HipGradientGaussianProcess([None] * 2, [None] * 2, [None] * 2, [None] * 2)
    m = B.HipTransformedModel(base, B.DeviceInputTransform(win, 2, 2), B.DeviceSlicedOutputTransform(fw, bw))
    assert m.gradient_base and m.warp is not None and m.sliceable
    rng = np.random.default_rng(12)
    X = rng.uniform(0.2, 1.2, (2, 7))
    X_ = np.array([win(X[:, j]) for j in range(7)]).T
    g = lambda z: np.array([np.sin(z[0]) + z[1] ** 2, z[0] * z[1]])                              # noqa: E731
    dg = lambda z: np.array([[np.cos(z[0]), 2 * z[1]], [z[1], z[0]]])                            # noqa: E731
    Y_ = np.array([g(X_[:, j]) for j in range(7)]).T
    Y = np.stack([a * Y_[i] + b for i, (a, b) in enumerate(W.AFFINE)])
    J = [np.array([[1 / (x[0] + 0.1), 0.0], [0.5 / (x[1] + 0.5 * x[0] + 0.1), 1 / (x[1] + 0.5 * x[0] + 0.1)]]) for x in X.T]
    dY = np.stack([np.diag([a for a, _ in W.AFFINE]) @ dg(X_[:, j]) @ J[j] for j in range(7)], axis=2)
    td = m.transform_data(B.GradientData(X, Y, dY))
    assert isinstance(td, B.GradientData) and np.array_equal(td.X, X_)
    assert np.abs(td.Y - Y_).max() <= 1e-15 * np.abs(Y_).max()
    want = np.stack([dg(X_[:, j]) for j in range(7)], axis=2)
    assert np.abs(td.dY - want).max() <= 1e-13 * np.abs(want).max()
    only_out = B.HipTransformedModel(base, None, B.DeviceSlicedOutputTransform(fw, bw)).transform_data(B.GradientData(X, Y, dY))
    assert np.abs(only_out.dY - np.stack([dg(X_[:, j]) @ J[j] for j in range(7)], axis=2)).max() <= 1e-13 * np.abs(dY).max()
    none = B.HipTransformedModel(base)
    gd = B.GradientData(X, Y, dY)
    assert none.transform_data(gd) is gd
    # what cannot carry gradient observations is refused with the reason
    with pytest.raises(NotImplementedError, match="plain closure has no derivative"):
        B.HipTransformedModel(base, B.InputTransform(win))
    with pytest.raises(NotImplementedError, match="plain closure has no derivative"):
        B.HipTransformedModel(base, None, B.SlicedOutputTransform(fw, bw))
    with pytest.raises(ValueError, match="square"):
        B.HipTransformedModel(base, B.DeviceInputTransform(W.in_closure("feature-log"), 2, 3))
