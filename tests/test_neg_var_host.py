"""The inputs of tests/test_gpu_neg_var.py, measured without a device, so that the GPU tests rest on nothing unmeasured
(tests/neg_var_cases.py describes both constructions).

Construction A: `flagged` traces within the limits and passes trace_kernel's checks; per case cond(K) is below the suite's 1e6 cap
and equals the figure the case was designed at; K* of every far candidate is exactly 0 under the library's own interpreter
(boss_kern_eval_host: the function the kernels call); the far variances hit their targets within FAR_BAR·α̃², with the candidates
scaled by division (the restatement) and by the device's multiply-by-reciprocal (scale_cand_kernel), so in-band targets stay in the
band and offending ones below it; the healthy variances are far from the band (measured: 3.1e-5 at N = 1030 to 8.2e-2 at
N = 20); the offenders are where the GPU test's table puts them, and every clip_var_kernel launch of more than one 256-thread
block has offenders in two blocks, the first not in the last.

Construction B (N = 40 / 130 / 1030, three kernels, two seeds): cond(K), the float64 restatement's midpoint variances, its share of
offending training-point candidates and its first offender are printed; asserted is what the GPU test needs of its inputs: cond <= 1.32,
every midpoint variance far above zero, no restated variance in the clip band (each is a multiple of ulp(1e10) = 1.9e-6), and both
offending and non-offending training-point candidates exist."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neg_var_cases as NV  # noqa: E402

COND = {"n20": 5.0e3, "n130": 3.2e4, "n130b": 3.2e4, "n130a3": 2.8e5, "n1030": 2.4e5}    # the figures the cases were designed at


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    return B


def test_flagged_traces_and_passes_the_tracer_checks(B):
    dk = B.DeviceKernel(NV.flagged, 3)                       # (trace_kernel raises ValueError on a failed value or symmetry check)
    prog = dk.program
    assert prog.d == 3 and prog.code.shape[0] <= 64 and prog.consts.shape[0] <= 32
    rng = np.random.default_rng(7)
    U, V = rng.standard_normal((3, 200)), rng.standard_normal((3, 200))
    want = np.array([float(NV.flagged(U[:, k], V[:, k])) for k in range(200)])
    host = prog.eval_host(U, V)
    print(f"[negvar-host] flagged: {prog.code.shape[0]} instructions, {prog.consts.shape[0]} constants, "
          f"max|eval_host - closure| {np.abs(host - want).max():.3e}, max|f(u,v) - f(v,u)| {np.abs(host - prog.eval_host(V, U)).max():.3e}")
    assert np.all(np.abs(host - want) <= 1e-14 * np.maximum(1.0, np.abs(want)))
    assert np.array_equal(host, prog.eval_host(V, U))        # symmetric to the bit: (u − v)² and u·v commute


@pytest.mark.parametrize("name", sorted(NV.A_CASES))
def test_construction_a(B, name):
    c = NV.case_a(name)
    ref = c.ref
    prog = B.DeviceKernel(NV.flagged, 3).program
    assert ref.cond < 1e6 and abs(ref.cond / COND[name] - 1) < 0.02, ref.cond
    assert c.off == NV.A_OFFENDERS[name] and c.off[0] >= (32 if c.M > 32 else 1)
    blocks = sorted({j // 256 for j in c.off})
    if c.M > 256:
        assert len(blocks) >= 2 and blocks[0] < (c.M - 1) // 256, blocks
    lamp = c.lam + 1e-8
    far = np.flatnonzero(c.far)
    H = np.array([j for j, k in enumerate(c.kinds) if k == "H"])
    P = np.array([j for j, k in enumerate(c.kinds) if k == "P"], dtype=int)
    scalings = {"division": c.Xs / lamp[:, None], "reciprocal": c.Xs * (1.0 / lamp)[:, None]}
    Ut = c.X * (1.0 / lamp)[:, None]
    lines = []
    for how, Us in scalings.items():
        # K* of the far candidates against every training point, by the library's interpreter: exactly zero
        uf = np.repeat(Us[:, far], c.N, axis=1)
        ut = np.tile(Ut, (1, far.size))
        ks = c.a2 * prog.eval_host(ut, uf)
        assert np.all(ks == 0.0), (how, np.abs(ks).max())
        var = c.a2 * prog.eval_host(Us[:, far], Us[:, far]) + NV.JITTER
        for j, v in zip(far, var):
            t = c.kinds[j]
            assert abs(v - t) <= NV.FAR_BAR * c.a2, (how, j, t, v)
            assert (v < -NV.MAX_NEG_VAR) == (t < -NV.MAX_NEG_VAR) and (v < 0.0) == (t < 0.0), (how, j, t, v)
        lines.append(f"{how} " + " ".join(f"{j}:{v!r}" for j, v in zip(far, var)))
    # the restatement itself: the same far variances, μ = 0 there, healthy variances far from the band, P far below it
    for j in far:
        assert abs(ref.var[j] - c.kinds[j]) <= NV.FAR_BAR * c.a2 and ref.mu[j] == 0.0, (j, ref.var[j], ref.mu[j])
    assert ref.var[H].min() >= 3e-5 and ref.var[H].max() < c.a2, (ref.var[H].min(), ref.var[H].max())
    if P.size:
        assert np.all(ref.var[P] < -1.25 * c.a2) and np.all(ref.var[P] >= -2.25 * c.a2), ref.var[P]
    assert sorted(NV.offenders(c.want_var)) == c.off and NV.offenders(c.want_var_clean).size == 0
    assert np.all(c.want_var[far][(c.want_var[far] < 0)] < -NV.MAX_NEG_VAR)        # expected values hold no band entry
    print(f"[negvar-host] A {name}: N {c.N} M {c.M} amp {c.amp} cond {ref.cond:.3e} tol {ref.tol:.3e} offenders {c.off} "
          f"H var [{ref.var[H].min():.3e}, {ref.var[H].max():.3e}] P var {list(ref.var[P])}")
    for ln in lines:
        print(f"[negvar-host]   far variances, {ln}")


@pytest.mark.parametrize("N", [40, 130, 1030])
def test_construction_b(N):
    for kernel in sorted(NV.K.BUILTIN):
        for seed in (1, 2):
            c = NV.case_b(N, kernel, seed)
            var = c.ref.var
            train = var[NV.N_MID:]
            off = NV.offenders(var)
            band = (var < 0.0) & (var >= -NV.MAX_NEG_VAR)
            share = float((train < -NV.MAX_NEG_VAR).mean())
            print(f"[negvar-host] B N {N} {kernel} seed {seed}: cond {c.ref.cond:.4f} B {c.B:.3e} midpoint var >= {var[:NV.N_MID].min():.3e} "
                  f"offenders {off.size} ({share:.1%} of the training-point candidates) first {int(off[0]) if off.size else -1} "
                  f"smallest |var| at a training point {np.abs(train).min():.3e}")
            assert c.ref.cond <= 1.32
            assert var[:NV.N_MID].min() >= 1e9               # no midpoint is anywhere near offending
            assert not band.any()
            assert off.size and off[0] >= NV.N_MID and (train >= 0.0).any()
            # the quantum: every restated training-point variance is a multiple of ulp(1e10) (plus the 1e-18 jitter where it is 0)
            q = np.spacing(1e10)
            assert q == 2.0 ** -19 and np.all(np.abs(train / q - np.rint(train / q)) <= 1e-9)
