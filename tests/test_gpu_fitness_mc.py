"""Monte-Carlo Expected Improvement of a fitness program on the device (boss_acq_ei_mc*), pytest -m gpu.

Value reference: the untouched host path acquisition.acquisition_nonlin with the closure.  Tolerance 1e-12 · max(1, max|f| + |best|):
two float64 evaluations of a well-conditioned program of <= 20 ops differ by <~ 20 · 2 ulp ≈ 1e-14 and the mean over k does not grow
that; the bound leaves ×100.  (The host path's Python max(0.0, NaN) is 0.0 and its sqrt of a negative variance is NaN, so the NaN,
clip and -Inf conventions are asserted directly, on candidates the reference is given sanitised moments for.)
Gradient reference: the formula of include/bosship.h in numpy from FitnessProgram.grad (fitness_mc_cases.ref_value_and_grad), at
1e-11 · max(1, max|∇acq|).  Gradient tests first assert, on the reference side, that no (candidate, ε) sits within 1e-9 of the
indicator's threshold or of a kink of F3.
"""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fitness_mc_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"both": (True, True), "best_only": (True, False), "cons_only": (False, True), "none": (False, False)}
FIT_OF_P = {1: "G1", 2: "F1", 3: "F3", 16: "F5"}


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd
    boss_jl_amd.api.load_library()
    assert boss_jl_amd.api.device_count() >= 1
    return boss_jl_amd


@pytest.fixture(scope="module")
def api(B):
    return B.api


@pytest.fixture(scope="module")
def fits(B):
    return {name: B.DeviceFitness(f, P) for name, (f, P) in cases.F.items()}


def vtol(prog, mu, var, eps, best):
    fmax = max(np.abs(f).max() for f in cases.f_values(prog, mu, cases.clip(var), eps))
    return 1e-12 * max(1.0, fmax + abs(0.0 if best is None else best))


def host_value(fit, mu, var, eps, y_max, best, mask):
    from boss_jl_amd import acquisition as acq_host
    return acq_host.acquisition_nonlin(fit, [(mu[s], var[s]) for s in range(mu.shape[0])], y_max, best, eps, mask)


def y_max_for(P):
    ym = np.linspace(0.4, 1.2, P)
    if P > 1:
        ym[0] = np.inf
    return ym


def value_case(fits, name, S, M, K, seed, special=True):
    """Moments with the special candidates of the issue: one variance of -1e-9 (clipped), one of -1e-6 (-Inf), mask zeros."""
    dfit = fits[name]
    P = dfit.y_dim
    mu, var = cases.moments(seed, S, P, M)
    eps = cases.eps_for(seed + 1, S, P, K)
    mask = np.ones(M, bool)
    jc = jp = None
    if special and M > 8:
        mask[[2, M - 1]] = False
        jc, jp = 4, 6
        var[0, 0, jc] = -1e-9
        var[S - 1, P - 1, jp] = -1e-6
    return dfit, mu, var, eps, mask, jc, jp


def check_value(api, fits, name, S, M, K, mode, seed):
    dfit, mu, var, eps, mask, jc, jp = value_case(fits, name, S, M, K, seed)
    has_best, cons = MODES[mode]
    best = 0.15 if has_best else None
    ym = y_max_for(dfit.y_dim) if cons else None
    acq, am, mx = api.acq_ei_mc_moments(mu, var, dfit.program, eps, ym, best, mask)
    acq2, am2, mx2 = api.acq_ei_mc_moments(mu, var, dfit.program, eps, ym, best, mask)
    assert np.array_equal(acq, acq2, equal_nan=True) and am == am2 and (mx == mx2)          # bit-identical on repeat
    safe = cases.clip(var)
    if jp is not None:
        safe[:, :, jp] = np.abs(safe[:, :, jp])
    ref = host_value(dfit, mu, safe, eps, ym, best, mask)
    tol = vtol(dfit.program, mu, safe, eps, best)
    ok = np.ones(M, bool)
    if jp is not None and (has_best or cons):
        ok[jp] = False
        assert acq[jp] == -np.inf                                 # a variance below the clip poisons the candidate
    err = np.abs(acq - ref)[ok].max()
    print(f"{name} S={S} M={M} K={K} {mode}: max|acq - ref| = {err:.3e} (tol {tol:.3e})")
    assert err <= tol
    assert np.all(acq[~mask] == 0.0)
    assert am == int(np.argmax(acq)) and mx == acq[am]            # first index of the maximum


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("P", [1, 3, 16])
@pytest.mark.parametrize("M", [1, 255, 257, 1025])
def test_moments_value_shapes_and_eps_counts(api, fits, M, P, S):
    for K in ((1, 7, 64, 65, 200) if S == 1 else (3,)):           # (S > 1: one ε column per sample, n_eps = S)
        check_value(api, fits, FIT_OF_P[P], S, M, K, "both", 100 * M + 10 * P + S)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("S", [1, 3])
def test_moments_value_modes(api, fits, S, mode):
    for P in (1, 3, 16):
        check_value(api, fits, FIT_OF_P[P], S, 257, 7, mode, 7000 + P + S)
    if mode == "none":
        dfit, mu, var, eps, mask, _, _ = value_case(fits, "F3", S, 257, 7, 1)
        acq, am, mx = api.acq_ei_mc_moments(mu, var, dfit.program, eps, None, None, mask)
        assert np.all(acq == 0.0) and am == 0 and mx == 0.0


@pytest.mark.parametrize("name", ["F1", "F2", "F4", "F6"])
def test_moments_value_every_opcode(api, fits, name):
    for S in (1, 3):
        check_value(api, fits, name, S, 257, 65, "both", 8000 + S)


def test_all_equal_acquisition_and_nan(api, B, fits):
    dfit, mu, var, eps, _, _, _ = value_case(fits, "F1", 1, 300, 64, 5, special=False)
    acq, am, mx = api.acq_ei_mc_moments(mu, var, dfit.program, eps, None, 10.0, None)     # best above every f (|F1| <= 2)
    assert np.all(acq == 0.0) and am == 0 and mx == 0.0
    # LOG of a negative number: NaN at that candidate, which the arg-max ranks largest
    lg = B.DeviceFitness(lambda y: np.log(y[0]), 1)
    mu1, var1 = np.full((1, 1, 40), 2.0), np.zeros((1, 1, 40))
    mu1[0, 0, 17] = -1.0
    acq, am, mx = api.acq_ei_mc_moments(mu1, var1, lg.program, np.zeros((1, 5)), None, 0.1, None)
    assert np.isnan(acq[17]) and am == 17 and np.isnan(mx)
    assert np.all(np.abs(np.delete(acq, 17) - (np.log(2.0) - 0.1)) <= 1e-15)


# ------------------------------------------------------------------------------------------ gradient from moments
def guard(dfit, name, mu, var, eps, best):
    """No (candidate, ε) within 1e-9 of the indicator's threshold, none on a kink of F3."""
    S, P, M = mu.shape
    for s, f in enumerate(cases.f_values(dfit.program, mu, cases.clip(var), eps)):
        assert np.abs(f - best).min() > 1e-9
        if name == "F3":
            e = eps if S == 1 else eps[:, s:s + 1]
            Y = mu[s][:, :, None] + np.sqrt(np.maximum(var[s], 0.0))[:, :, None] * e[:, None, :]
            assert np.abs(Y[0] - Y[1]).min() > 1e-9 and np.abs(Y[2]).min() > 1e-9


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F5"])
@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("M", [1, 65, 224])
def test_moments_gradient_against_the_formula(api, fits, M, d, name, S):
    dfit = fits[name]
    P, K, best = dfit.y_dim, 37, 0.15
    mu, var, dmu, dvar = cases.moments(300 + M + d + S, S, P, M, d)
    eps = cases.eps_for(900 + M + d, S, P, K)
    mask = np.ones(M, bool)
    jc = jp = None
    if M > 8:
        mask[[2, M - 1]] = False
        jc, jp = 4, 6
        var[0, 0, jc] = -1e-9                                     # clipped: no σ term from this output
        var[S - 1, P - 1, jp] = -1e-6                             # poisoned: -Inf, gradient 0
    ym = y_max_for(P)
    guard(dfit, name, mu, var, eps, best)
    acq, dacq = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, dfit.program, eps, ym, best, mask)
    acq2, dacq2 = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, dfit.program, eps, ym, best, mask)
    assert np.array_equal(acq, acq2) and np.array_equal(dacq, dacq2)
    ra, rg = cases.ref_value_and_grad(dfit.program, mu, var, dmu, dvar, eps, ym, best, mask)
    ok = np.isfinite(ra)
    tol_v = vtol(dfit.program, mu, var, eps, best)
    tol_g = 1e-11 * max(1.0, np.abs(rg).max())
    print(f"{name} S={S} M={M} d={d}: max|Δacq| = {np.abs(acq - ra)[ok].max():.3e} (tol {tol_v:.3e}), "
          f"max|Δ∇acq| = {np.abs(dacq - rg).max():.3e} (tol {tol_g:.3e})")
    assert np.array_equal(np.isfinite(acq), ok) and np.abs(acq - ra)[ok].max() <= tol_v
    assert np.abs(dacq - rg).max() <= tol_g
    assert np.all(dacq[:, ~mask] == 0.0) and np.all(acq[~mask] == 0.0)
    if jp is not None:
        assert acq[jp] == -np.inf and np.all(dacq[:, jp] == 0.0)
        # the clipped variance contributes no σ term: its ∇σ² may be anything
        dvar2 = dvar.copy()
        dvar2[0, 0, :, jc] = 1e6
        _, dacq3 = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar2, dfit.program, eps, ym, best, mask)
        assert np.array_equal(dacq3[:, jc], dacq[:, jc])
    for mode in ("best_only", "cons_only", "none"):
        hb, cons = MODES[mode]
        a, g = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, dfit.program, eps, ym if cons else None, best if hb else None, mask)
        ra, rg = cases.ref_value_and_grad(dfit.program, mu, var, dmu, dvar, eps, ym if cons else None, best if hb else None, mask)
        ok = np.isfinite(ra)
        assert np.array_equal(np.isfinite(a), ok) and np.abs(a - ra)[ok].max() <= tol_v, mode
        assert np.abs(g - rg).max() <= 1e-11 * max(1.0, np.abs(rg).max()), mode


# ------------------------------------------------------------------------------------------ gradient: the branches of workload sizes
ALL_MODES = ("both", "best_only", "cons_only", "none")
SPECIAL_65 = ((2, 64), 4, 6)                                      # (masked, clipped, poisoned) of the test above at M = 65
SPECIAL_5 = ((1,), 2, 3)


def grad_case(dfit, name, S, M, d, K, seed, special=None, best=0.15):
    """Seeded inputs of a gradient test; `special` = (masked candidates, the one with a variance of -1e-9, the one with -1e-6).
    The guard is asserted here, on the inputs: choosing a seed needs no device."""
    P = dfit.y_dim
    mu, var, dmu, dvar = cases.moments(seed, S, P, M, d)
    eps = cases.eps_for(seed + 1, S, P, K)
    mask = np.ones(M, bool)
    jc = jp = None
    if special is not None:
        masked, jc, jp = special
        mask[list(masked)] = False
        var[0, 0, jc] = -1e-9
        var[S - 1, P - 1, jp] = -1e-6
    guard(dfit, name, mu, var, eps, best)
    return mu, var, dmu, dvar, eps, mask, jc, jp


def check_grad(api, dfit, label, case, best=0.15, modes=ALL_MODES):
    """Value and gradient of the gradient kernel against the formula in every mode of `modes`, bit-identical on repeat; only the poisoned
    candidate is exempt from the value comparison (it must be -Inf with gradient 0).  Returns the largest errors seen."""
    mu, var, dmu, dvar, eps, mask, jc, jp = case
    ym_all = y_max_for(dfit.y_dim)
    tol_v = vtol(dfit.program, mu, var, eps, best)
    worst_v = worst_g = 0.0
    for mode in modes:
        hb, cons = MODES[mode]
        ym, b = ym_all if cons else None, best if hb else None
        acq, dacq = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, dfit.program, eps, ym, b, mask)
        acq2, dacq2 = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, dfit.program, eps, ym, b, mask)
        assert np.array_equal(acq, acq2) and np.array_equal(dacq, dacq2), mode
        ra, rg = cases.ref_value_and_grad(dfit.program, mu, var, dmu, dvar, eps, ym, b, mask)
        ok = np.isfinite(ra)
        tol_g = 1e-11 * max(1.0, np.abs(rg).max())
        with np.errstate(invalid="ignore"):                     # (-Inf minus -Inf at the poisoned candidate, left out by `ok`)
            ev, eg = np.abs(acq - ra)[ok].max(), np.abs(dacq - rg).max()
        print(f"{label} {mode}: max|Δacq| = {ev:.3e} (tol {tol_v:.3e}), max|Δ∇acq| = {eg:.3e} (tol {tol_g:.3e})")
        assert np.array_equal(np.isfinite(acq), ok) and ev <= tol_v, mode
        assert eg <= tol_g, mode
        assert np.all(dacq[:, ~mask] == 0.0) and np.all(acq[~mask] == 0.0), mode
        if jp is not None and mode != "none":
            assert int((~ok).sum()) == 1 and acq[jp] == -np.inf and np.all(dacq[:, jp] == 0.0), mode
        else:
            assert ok.all(), mode
        worst_v, worst_g = max(worst_v, ev / tol_v), max(worst_g, eg / tol_g)
    return worst_v, worst_g


@pytest.mark.parametrize("K", [64, 65, 128, 200])
@pytest.mark.parametrize("name", ["F2", "F3", "F5"])
@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("M", [1, 65])
def test_moments_gradient_at_the_workload_eps_counts(api, fits, M, d, name, K):
    """One posterior sample, 64 to 200 ε: one to four passes of the lanes over k, the A / B sums carried across passes, lanes busy in
    one pass and idle in the next (K = 65, 200), in a four-wave (F2, F3) and a one-wave (F5) workgroup.
    Observed over the 48 cases and four modes: max|Δacq| = 4.4e-16 (tol >= 1.4e-12), max|Δ∇acq| = 1.1e-14 (tol 1e-11 to 3.5e-10)."""
    case = grad_case(fits[name], name, 1, M, d, K, 4000 + 10 * K + M + d, SPECIAL_65 if M > 8 else None)
    check_grad(api, fits[name], f"{name} S=1 M={M} d={d} K={K}", case)


@pytest.mark.parametrize("name", ["F2", "F3", "F5"])
def test_moments_gradient_sums_start_afresh_for_every_sample(api, fits, name):
    """S = 3, M = 65: one ε column per sample (K = 1 inside the wave); sums left over from the sample before would show in the next.
    Observed: max|Δacq| = 3.3e-16 (tol >= 2.2e-12), max|Δ∇acq| = 4.4e-16 (tol >= 1e-11)."""
    case = grad_case(fits[name], name, 3, 65, 8, 3, 4700, SPECIAL_65)
    check_grad(api, fits[name], f"{name} S=3 M=65 d=8", case)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("d", [64, 65, 130])
def test_moments_gradient_wide_x(api, fits, d, S):
    """One, two and three passes of the lanes over the coordinates (the zeroing, the assembly and the final division), one masked
    and one poisoned candidate among five.  Observed: max|Δacq| = 2.8e-17 (tol >= 1.7e-12), max|Δ∇acq| = 1.1e-16 (tol 1e-11)."""
    case = grad_case(fits["F3"], "F3", S, 5, d, 65, 4800 + d + S, SPECIAL_5)
    check_grad(api, fits["F3"], f"F3 S={S} M=5 d={d} K=65", case, modes=("both",))


# ------------------------------------------------------------------------------------------ workgroup shapes
SHAPE_PROGRAM = {False: {1: "F5", 2: "W2v", 3: "W3v", 4: "F1"}, True: {1: "F5", 2: "F4", 3: "W3g", 4: "F1"}}     # [gradient kernel?][waves]


def test_the_closures_reach_every_workgroup_shape(fits):
    """The launch rule (mc_block) on the traced programs' P and instruction counts: both kernels run with 1, 2, 3 and 4 waves."""
    for grad in (False, True):
        seen = {}
        for name, dfit in fits.items():
            p = dfit.program
            seen.setdefault(cases.mc_waves(p.P, p.code.shape[0], grad), []).append(name)
        print("gradient kernel" if grad else "value kernel", {w: seen[w] for w in sorted(seen)})
        assert sorted(seen) == [1, 2, 3, 4]
        for w, name in SHAPE_PROGRAM[grad].items():
            assert name in seen[w]
    # the rule itself at its edges: 32 | 33, 42 | 43, 64 | 65 slots
    assert [cases.mc_waves(1, s - 3, False) for s in (32, 33, 42, 43, 64, 65)] == [4, 3, 3, 2, 2, 1]
    assert [cases.mc_waves(1, (s - 6) // 2, True) for s in (32, 34, 42, 44, 64, 66)] == [4, 3, 3, 2, 2, 1]


@pytest.mark.parametrize("waves", [1, 2, 3, 4])
@pytest.mark.parametrize("grad", [False, True], ids=["value", "gradient"])
def test_every_workgroup_shape(api, fits, grad, waves):
    """A lone candidate, a second block of one wave, a third block of one wave: j = blockIdx.x · waves + wave and the exit of the
    waves behind the last candidate, for workgroups of 64, 128, 192 and 256 threads.
    Observed: value max|acq - ref| = 1.1e-16 (tol >= 1e-12); gradient max|Δacq| = 4.4e-16 (tol >= 1.4e-12), max|Δ∇acq| = 8.9e-16 (tol >= 1e-11)."""
    name = SHAPE_PROGRAM[grad][waves]
    p = fits[name].program
    assert cases.mc_waves(p.P, p.code.shape[0], grad) == waves
    for M in (1, waves + 1, 2 * waves + 1):
        if grad:
            case = grad_case(fits[name], name, 1, M, 2, 65, 5000 + 10 * waves + M, SPECIAL_5 if M >= 5 else None)
            check_grad(api, fits[name], f"{name} waves={waves} M={M}", case, modes=("both",))
        else:
            check_value(api, fits, name, 1, M, 65, "both", 5100 + 10 * waves + M)


# ------------------------------------------------------------------------------------------ program size limits
BIG_BEST = 0.05


@pytest.mark.parametrize("S", [1, 3])
def test_largest_program(api, S):
    """16 inputs, 32 constants, 64 instructions (cases.big_program): 56 KiB of LDS in the value kernel, the 112 KiB the gradient
    kernel is allowed at most.  Observed: value 5.6e-17 (tol >= 1.3e-12); gradient max|Δacq| = 1.1e-16 (tol >= 1e-12), max|Δ∇acq| = 3.3e-16 (tol 1e-11)."""
    big = cases.HandFitness(cases.big_program(api))
    p = big.program
    assert cases.mc_slots(p.P, p.code.shape[0], True) * 512 == 112 * 1024
    check_value(api, {"BIG": big}, "BIG", S, 3, 65, "both", 5200 + S)
    case = grad_case(big, "BIG", S, 3, 2, 65, 5210 + S, best=BIG_BEST)
    f = np.concatenate([x.ravel() for x in cases.f_values(p, case[0], case[1], case[4])])
    assert 0.2 <= (f > BIG_BEST).mean() <= 0.8                    # the indicator is on for some ε and off for others
    check_grad(api, big, f"BIG S={S} M=3 d=2", case, best=BIG_BEST)


@pytest.mark.parametrize("out_id", [1, 2], ids=["input", "constant"])
def test_empty_programs(api, out_id):
    """No instruction: the value is an input (f = y_1) or a constant (f = 0.7, ∇f = 0: ∇acq = EI ∇FP, and exactly 0 without constraints).
    Observed: value 3.9e-16 (tol >= 1e-12); gradient max|Δacq| = 2.2e-16 (tol >= 1e-12), max|Δ∇acq| = 1.1e-16 (tol 1e-11)."""
    fit = cases.HandFitness(api.FitnessProgram(2, [0.7], [], out_id))
    for S in (1, 3):
        check_value(api, {"E": fit}, "E", S, 3, 65, "both", 5300 + S)
        case = grad_case(fit, "E", S, 3, 2, 65, 5310 + S)
        check_grad(api, fit, f"empty out_id={out_id} S={S}", case)
    if out_id == 2:
        mu, var, dmu, dvar, eps, mask, _, _ = grad_case(fit, "E", 1, 3, 2, 65, 5311)
        ym, best = y_max_for(2), 0.15
        a_both, g_both = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, fit.program, eps, ym, best, mask)
        fp, dfp = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, fit.program, eps, ym, None, mask)
        a_best, g_best = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, fit.program, eps, None, best, mask)
        assert np.all(g_best == 0.0) and np.all(np.abs(a_best - (0.7 - best)) <= vtol(fit.program, mu, var, eps, best))
        assert np.abs(g_both - (0.7 - best) * dfp).max() <= 1e-11 * max(1.0, np.abs(g_both).max())
        assert np.abs(a_both - (0.7 - best) * fp).max() <= vtol(fit.program, mu, var, eps, best)


# ------------------------------------------------------------------------------------------ the reverse sweep on the device
def device_gradient(api, prog, Y):
    """(f, ∇f) at the columns of Y (P×n) read off the gradient kernel: one posterior sample, σ² = 0 and ε = 0 so y = μ exactly and no σ
    term arises, ∇μ_p = e_p (d = P), no constraint, best = -1e3 below every value: acq = f - best, ∇acq = ∇f."""
    P, n = Y.shape
    dmu = np.zeros((1, P, P, n))
    for p in range(P):
        dmu[0, p, p, :] = 1.0
    acq, dacq = api.acq_ei_mc_grad_moments(Y[None], np.zeros((1, P, n)), dmu, np.ones((1, P, P, n)), prog, np.zeros((P, 1)), None, -1e3, None)
    return acq, dacq


def test_reverse_sweep_conventions_on_the_device(api):
    """Every opcode through fit_grad as the device runs it (slots strided in LDS, the device's libm), against boss_fit_eval_host at the
    same points; test_fitness_program_host.py pins that function's conventions to their literal values.  Equality for the arithmetic
    opcodes and the conventions; DIV and the libm opcodes at 1e-12 · max(1, |f| + |best|) and 1e-11 · max(1, max|∇f|).
    A partial derivative of ±Inf is read with P = d = 1 (with more inputs the identity ∇μ makes Inf · 0 = NaN elsewhere, as IEEE says).
    Observed for the opcodes under a tolerance: max|Δf| = 0 (tol 1e-9), max|Δ∇f| = 8.9e-16 (EXP at 1.7; tol 5.5e-11), 0 for the others."""
    op = api.FIT_OP
    un = lambda name: (1, [], [[op[name], 0, -1]], 1)             # noqa: E731
    bi = lambda name: (2, [], [[op[name], 0, 1]], 2)              # noqa: E731
    exact = [
        ("ABS", un("ABS"), [[0.0, 1.5, -1.5]]),                                      # ABS'(0) = 0
        ("NEG", un("NEG"), [[1.5, -3.0]]),
        ("SQUARE", un("SQUARE"), [[1.5, -3.0]]),
        ("SQRT", un("SQRT"), [[0.0, 4.0]]),                                          # SQRT'(0) = +Inf
        ("ADD", bi("ADD"), [[1.5], [2.0]]),
        ("SUB", bi("SUB"), [[1.5], [2.0]]),
        ("MUL", bi("MUL"), [[1.5], [2.0]]),
        ("MIN", bi("MIN"), [[1.0, 2.0, 1.0], [2.0, 1.0, 1.0]]),                      # ordered both ways, tied: the first operand
        ("MAX", bi("MAX"), [[1.0, 2.0, 1.0], [2.0, 1.0, 1.0]]),
        ("POW const", (1, [3.0], [[op["POW"], 0, 1]], 2), [[-2.0]]),                 # no ∂/∂b term, no NaN
        ("POW var", bi("POW"), [[2.0], [3.0]]),                                      # ∂/∂b = r log(a)
        ("dead branch", (2, [0.0], [[op["SQRT"], 0, -1], [op["MUL"], 3, 2], [op["ADD"], 4, 1]], 5), [[0.0], [0.7]]),
    ]
    for label, spec, pts in exact:
        prog = api.FitnessProgram(*spec)
        Y = np.array(pts, float)
        f, df = prog.eval_host(Y, want_grad=True)
        acq, dacq = device_gradient(api, prog, Y)
        print(f"{label}: f = {acq - 1e3}, ∇f = {dacq.tolist()} (host {df.tolist()})")
        assert np.array_equal(acq, f + 1e3), label
        assert np.array_equal(dacq, df), label
    # spelled out where a convention decides (the host test holds boss_fit_eval_host to the same literals)
    _, g = device_gradient(api, api.FitnessProgram(*exact[0][1]), np.array([[0.0, 1.5, -1.5]]))
    assert g.tolist() == [[0.0, 1.0, -1.0]]
    _, g = device_gradient(api, api.FitnessProgram(*exact[3][1]), np.array([[0.0]]))
    assert g[0, 0] == np.inf
    _, g = device_gradient(api, api.FitnessProgram(*exact[7][1]), np.array(exact[7][2]))
    assert g.tolist() == [[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]]
    _, g = device_gradient(api, api.FitnessProgram(*exact[8][1]), np.array(exact[8][2]))
    assert g.tolist() == [[0.0, 1.0, 1.0], [1.0, 0.0, 0.0]]
    a, g = device_gradient(api, api.FitnessProgram(*exact[9][1]), np.array([[-2.0]]))
    assert a[0] == 992.0 and g[0, 0] == 12.0
    a, g = device_gradient(api, api.FitnessProgram(*exact[11][1]), np.array([[0.0], [0.7]]))
    assert a[0] == 0.7 + 1e3 and g[:, 0].tolist() == [0.0, 1.0]      # the adjoint 0 of SQRT passes nothing on: no 0 · Inf
    worst_f = worst_g = 0.0
    for label, spec, pts in [("DIV", bi("DIV"), [[3.0, -0.7], [2.0, 1.3]])] + \
                            [(n, un(n), [[0.3, 1.7]]) for n in ("EXP", "LOG", "SIN", "COS", "TANH", "SQRT")]:
        prog = api.FitnessProgram(*spec)
        Y = np.array(pts, float)
        f, df = prog.eval_host(Y, want_grad=True)
        acq, dacq = device_gradient(api, prog, Y)
        ef, eg = np.abs(acq - (f + 1e3)).max(), np.abs(dacq - df).max()
        tol_f, tol_g = 1e-12 * max(1.0, np.abs(f).max() + 1e3), 1e-11 * max(1.0, np.abs(df).max())
        print(f"{label}: max|Δf| = {ef:.3e} (tol {tol_f:.3e}), max|Δ∇f| = {eg:.3e} (tol {tol_g:.3e})")
        assert ef <= tol_f and eg <= tol_g, label
        worst_f, worst_g = max(worst_f, ef), max(worst_g, eg)
    print(f"libm opcodes: max|Δf| = {worst_f:.3e}, max|Δ∇f| = {worst_g:.3e}")


def test_nan_through_the_gradient_kernel(api, B):
    """LOG of a negative number at one candidate (μ = -1, σ = 0): its acquisition is NaN and its gradient 0 (a NaN value is no
    improvement and enters no sum); its neighbours match the formula.  Observed: max|Δacq| = 0 (tol 1e-12), max|Δ∇acq| = 1.1e-16 (tol 1e-11)."""
    lg = B.DeviceFitness(lambda y: np.log(y[0]), 1)
    M, d, K, best = 40, 2, 5, 0.1
    rng = np.random.default_rng(5400)
    mu, var = np.full((1, 1, M), 2.0), np.full((1, 1, M), 0.04)   # σ = 0.2: y > 0 for |ε| < 10
    mu[0, 0, 17], var[0, 0, 17] = -1.0, 0.0
    dmu, dvar = rng.uniform(-1, 1, (1, 1, d, M)), rng.uniform(-1, 1, (1, 1, d, M))
    eps = cases.eps_for(5401, 1, 1, K)
    others = np.arange(M) != 17
    f = cases.f_values(lg.program, mu[:, :, others], var[:, :, others], eps)[0]
    assert np.abs(f - best).min() > 1e-9 and (f > best).any()
    acq, dacq = api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, lg.program, eps, None, best, None)
    assert np.isnan(acq[17]) and np.all(dacq[:, 17] == 0.0)
    with np.errstate(all="ignore"):
        ra, rg = cases.ref_value_and_grad(lg.program, mu, var, dmu, dvar, eps, None, best, None)
    tol_v, tol_g = vtol(lg.program, mu[:, :, others], var[:, :, others], eps, best), 1e-11 * max(1.0, np.abs(rg[:, others]).max())
    ev, eg = np.abs(acq - ra)[others].max(), np.abs(dacq - rg)[:, others].max()
    print(f"LOG with one NaN candidate: max|Δacq| = {ev:.3e} (tol {tol_v:.3e}), max|Δ∇acq| = {eg:.3e} (tol {tol_g:.3e})")
    assert ev <= tol_v and eg <= tol_g


# ------------------------------------------------------------------------------------------ handles
def _data(seed, d, N):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[-1] + 0.2 * np.cos(4 * X[0])])
    return rng, X, Y


@pytest.fixture(scope="module")
def handle_sets(api):
    """name -> (gps[s][p], d): plain GPs at N = 40 and 300, gradient observations (n = 20, d = 2), a BI set of S = 3 from fit_batch."""
    out = {}
    for N in (40, 300):
        _, X, Y = _data(N, 3, N)
        out[f"plain{N}"] = ([[api.fit(X, Y[p], "matern52", [0.4, 0.5, 0.6], 1.0 + 0.2 * p, 0.05) for p in range(2)]], 3)
    rng, X, Y = _data(20, 2, 20)
    gg = []
    for p in range(2):
        dY = np.stack([3 * np.cos(3 * X[0]), 3 * np.cos(3 * X[1])]) if p == 0 else np.stack([1 - 0.8 * np.sin(4 * X[0]), -np.ones(20)])
        g = api.GradGP(X, Y[p], dY, "sqexp")
        g.update([0.5, 0.6], 1.1, 0.05, 0.1)
        gg.append(g)
    out["gradobs"] = ([gg], 2)
    rng, X, Y = _data(77, 3, 150)
    lam = rng.uniform(0.35, 0.8, (2, 3, 3))
    cols = [api.fit_batch(X, Y[p], "matern52", lam[p], rng.uniform(0.8, 1.5, 3), rng.uniform(0.04, 0.1, 3))[0] for p in range(2)]
    out["bi3"] = ([[cols[p][s] for p in range(2)] for s in range(3)], 3)
    yield out
    for gps, _ in out.values():
        for row in gps:
            for g in row:
                g.close()


@pytest.mark.parametrize("key", ["plain40", "plain300", "gradobs", "bi3"])
def test_handles_value_against_the_host_path(api, fits, handle_sets, key):
    gps, d = handle_sets[key]
    S, M = len(gps), 257
    dfit = fits["F1"]
    Xs = np.asfortranarray(np.random.default_rng(5).uniform(-0.05, 1.05, (d, M)))
    mask = np.all((Xs >= 0) & (Xs <= 1), axis=0)
    eps = cases.eps_for(6, S, 2, 64)
    mv = [[g.predict(Xs) for g in row] for row in gps]
    mu = np.stack([np.stack([r[0] for r in row]) for row in mv])
    var = np.stack([np.stack([r[1] for r in row]) for row in mv])
    ym, best = np.array([np.inf, 0.9]), 0.3
    cand = api.Candidates(Xs)
    acq, am, mx = api.acq_ei_mc(gps, cand, dfit.program, eps, ym, best, mask)
    _, am2, mx2 = api.acq_ei_mc(gps, cand, dfit.program, eps, ym, best, mask, want_acq=False)
    cand.close()
    ref = host_value(dfit, mu, cases.clip(var), eps, ym, best, mask)
    tol = vtol(dfit.program, mu, var, eps, best)
    print(f"{key}: max|acq - ref| = {np.abs(acq - ref).max():.3e} (tol {tol:.3e})")
    assert np.abs(acq - ref).max() <= tol
    assert am == int(np.argmax(acq)) and mx == acq[am] and (am2, mx2) == (am, mx)


@pytest.mark.parametrize("key", ["plain40", "plain300", "gradobs", "bi3"])
def test_handles_gradient_two_ways(api, fits, handle_sets, key):
    gps, d = handle_sets[key]
    S, M = len(gps), 65
    dfit = fits["F2"]
    Xs = np.asfortranarray(np.random.default_rng(8).uniform(0.05, 0.95, (d, M)))
    eps = cases.eps_for(9, S, 2, 50)
    ym, best = np.array([np.inf, 0.9]), -1.2
    acq, dacq = api.acq_ei_mc_grad(gps, Xs, dfit.program, eps, ym, best, None)
    acq2, dacq2 = api.acq_ei_mc_grad(gps, Xs, dfit.program, eps, ym, best, None)
    assert np.array_equal(acq, acq2) and np.array_equal(dacq, dacq2)
    # (1) the formula on the handles' predict_grad moments
    pg = [[g.predict_grad(Xs) for g in row] for row in gps]
    mu, var, dmu, dvar = (np.stack([np.stack([r[q] for r in row]) for row in pg]) for q in range(4))
    guard(dfit, "F2", mu, var, eps, best)
    ra, rg = cases.ref_value_and_grad(dfit.program, mu, var, dmu, dvar, eps, ym, best, None)
    tol_g = 1e-11 * max(1.0, np.abs(rg).max())
    print(f"{key}: max|Δacq| = {np.abs(acq - ra).max():.3e}, max|Δ∇acq| = {np.abs(dacq - rg).max():.3e} (tol {tol_g:.3e})")
    assert np.abs(acq - ra).max() <= vtol(dfit.program, mu, var, eps, best)
    assert np.abs(dacq - rg).max() <= tol_g
    # (2) central differences of acq_ei_mc's value with ε fixed, h = 1e-5: h² truncation plus 1e-12/h rounding ≈ 1e-7
    h = 1e-5
    fd = np.zeros((d, M))
    for m in range(d):
        vals = []
        for sgn in (1.0, -1.0):
            Xp = Xs.copy()
            Xp[m] += sgn * h
            cand = api.Candidates(Xp)
            vals.append(api.acq_ei_mc(gps, cand, dfit.program, eps, ym, best, None)[0])
            cand.close()
        fd[m] = (vals[0] - vals[1]) / (2 * h)
    print(f"{key}: max|fd - ∇acq| = {np.abs(fd - dacq).max():.3e} (tol {1e-6 * np.abs(dacq).max():.3e})")
    assert np.abs(fd - dacq).max() <= 1e-6 * np.abs(dacq).max()


def test_validation_leaves_the_handles_usable(api, fits, handle_sets):
    gps, d = handle_sets["bi3"]
    Xs = np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (d, 20)))
    cand = api.Candidates(Xs)
    good = cases.eps_for(2, 3, 2, 3)
    calls = [lambda fit, eps: api.acq_ei_mc(gps, cand, fit, eps, None, 0.1),
             lambda fit, eps: api.acq_ei_mc_grad(gps, Xs, fit, eps, None, 0.1),
             lambda fit, eps: api.acq_ei_mc_moments(np.zeros((3, 2, 20)), np.ones((3, 2, 20)), fit, eps, None, 0.1),
             lambda fit, eps: api.acq_ei_mc_grad_moments(np.zeros((3, 2, 20)), np.ones((3, 2, 20)), np.zeros((3, 2, d, 20)),
                                                         np.zeros((3, 2, d, 20)), fit, eps, None, 0.1)]
    nan_eps = good.copy()
    nan_eps[1, 2] = np.nan
    for call in calls:
        for fit, eps in [(fits["F3"].program, good),                                   # P mismatch
                         (fits["F1"].program, cases.eps_for(2, 1, 2, 5)),              # S = 3 with n_eps = 5
                         (fits["F1"].program, nan_eps)]:                               # NaN in ε
            with pytest.raises(api.BossError) as e:
                call(fit, eps)
            assert e.value.code == api.BOSS_E_INVALID
        call(fits["F1"].program, good)                                                 # ... and the handles still work
    a1 = api.acq_ei_mc(gps, cand, fits["F1"].program, good, None, 0.1)[0]
    assert np.all(np.isfinite(a1))
    cand.close()


# ------------------------------------------------------------------------------------------ end to end
def _problem(B, fit, params=None):
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, (2, 60))
    Y = np.stack([np.sin(3 * X[0]) + X[1], 0.5 * X[0] - X[1] ** 2])
    return B.BossProblem(f=None, domain=B.Domain(bounds=([0., 0.], [1., 1.])), y_max=[np.inf, 0.6],
                         acquisition=B.ExpectedImprovement(fit, eps_samples=40),
                         model=B.HipGaussianProcess(lengthscale_priors=[None] * 2, amplitude_priors=[None] * 2, noise_std_priors=[None] * 2),
                         data=B.ExperimentData(X, Y),
                         params=params or B.HipGPParams(np.full((2, 2), 0.4), [1.0, 1.0], [0.05, 0.05]))


def test_batch_maximiser_agrees_with_the_host_path(B, fits):
    f, P = cases.F["F1"]
    g1, g2 = np.meshgrid(np.linspace(-0.02, 1.02, 32), np.linspace(0.0, 1.0, 16))
    pts = np.asfortranarray(np.stack([g1.ravel(), g2.ravel()]))                        # 512 points, some outside the bounds
    am = B.HipBatchAM(points=pts)
    for params in (None, [B.HipGPParams(np.full((2, 2), 0.4), [1.0, 1.0], [0.05, 0.05]), B.HipGPParams(np.full((2, 2), 0.6), [1.2, 0.8], [0.05, 0.05])]):
        pd, pn = _problem(B, fits["F1"], params), _problem(B, B.NonlinFitness(f), params)
        xd, vd = am.maximize_acquisition(pd)
        xn, vn = am.maximize_acquisition(pn)
        _, ad = am.maximize_acquisition(pd, return_all=True)
        _, an = am.maximize_acquisition(pn, return_all=True)
        tol = 1e-12 * max(1.0, 2.0 + abs(B.problem.best_so_far(pn.acquisition.fitness, pn.data.Y, pn.y_max)))     # |F1| <= 2
        print(f"S={1 if params is None else 2}: max|acq_device - acq_host| = {np.abs(ad - an).max():.3e} (tol {tol:.3e})")
        assert np.abs(ad - an).max() <= tol
        assert np.array_equal(xd, xn) and abs(vd - vn) <= tol


def test_gradient_maximiser_with_a_device_fitness(B, fits):
    from boss_jl_amd.maximizer import posteriors_of
    prob = _problem(B, fits["F2"])
    prior = lambda r: r.uniform(0.0, 1.0, 2)                      # noqa: E731
    am = B.HipGradientAM(x_prior=prior, multistart=32, iters=10, seed=3)
    x, v = am.maximize_acquisition(prob)
    x2, v2 = am.maximize_acquisition(prob)
    assert np.array_equal(x, x2) and v == v2                      # the ε draw is seeded: identical on a second run
    assert np.all(x >= 0.0) and np.all(x <= 1.0)
    rng = np.random.default_rng(3)
    X0 = np.asfortranarray(np.stack([prior(rng) for _ in range(32)], axis=1))
    posts = posteriors_of(prob)
    f0, _ = am._value_and_grad(prob, posts, X0)                   # (eps_seed = 0: the same ε draw as inside the call above)
    for p in posts:
        p.close()
    assert v >= f0.max()                                          # the ascent never leaves a start below where it began
    with pytest.raises(NotImplementedError):
        am.maximize_acquisition(_problem(B, B.NonlinFitness(cases.F["F2"][0])))


def test_nonstationary_posterior(B, fits):
    """HipNonstationaryGP at N = 64: acquisition_values against the host path, HipGradientAM's value and gradient against the formula
    on the slices' mean_and_var_grad moments."""
    from boss_jl_amd.maximizer import _mc_eps, acquisition_values
    from boss_jl_amd.model import HipGaussianProcessPosterior
    rng = np.random.default_rng(4)
    d, N, M = 2, 64, 65
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3 * X[0]) + X[1], 0.5 * X[0] - X[1] ** 2])
    f_lam = lambda x: 0.4 + 0.2 * np.asarray(x) ** 2              # noqa: E731
    f_amp = lambda x: 1.0 + 0.3 * np.sin(np.sum(x))               # noqa: E731
    f_noise = lambda x: 0.05                                      # noqa: E731
    model = B.HipNonstationaryGP([f_lam] * 2, [f_amp] * 2, [f_noise] * 2)
    data = B.ExperimentData(X, Y)
    post = HipGaussianProcessPosterior(model.model_posterior(data))
    mk = lambda fit: B.BossProblem(f=None, domain=B.Domain(bounds=([0., 0.], [1., 1.])), y_max=[np.inf, 0.6],            # noqa: E731
                                   acquisition=B.ExpectedImprovement(fit, eps_samples=40), model=model, data=data)
    try:
        Xs = np.asfortranarray(rng.uniform(0.02, 0.98, (d, M)))
        pd, pn = mk(fits["F1"]), mk(B.NonlinFitness(cases.F["F1"][0]))
        ad, amd, mxd = acquisition_values(pd, [post], Xs)
        an, amn, _ = acquisition_values(pn, [post], Xs)
        best = B.problem.best_so_far(pn.acquisition.fitness, Y, pn.y_max)
        tol = 1e-12 * max(1.0, 2.0 + abs(best))
        print(f"nonstationary: max|acq_device - acq_host| = {np.abs(ad - an).max():.3e} (tol {tol:.3e})")
        assert np.abs(ad - an).max() <= tol and amd == amn and mxd == ad[amd]
        am = B.HipGradientAM(x_prior=lambda r: r.uniform(0.0, 1.0, 2), multistart=8, iters=3, seed=1)
        p2 = mk(fits["F2"])
        eps = _mc_eps(p2, 1, am.eps_seed)
        a, g = am._value_and_grad(p2, [post], Xs)
        pg = [s.mean_and_var_grad(Xs) for s in post.slices]
        mu, var, dmu, dvar = (np.stack([r[q] for r in pg])[None] for q in range(4))
        b2 = B.problem.best_so_far(p2.acquisition.fitness, Y, p2.y_max)
        guard(fits["F2"], "F2", mu, var, eps, b2)
        ra, rg = cases.ref_value_and_grad(fits["F2"].program, mu, var, dmu, dvar, eps, p2.y_max, b2, np.ones(M, bool))
        assert np.abs(a - ra).max() <= vtol(fits["F2"].program, mu, var, eps, b2)
        assert np.abs(g - rg).max() <= 1e-11 * max(1.0, np.abs(rg).max())
        x, v = am.maximize_acquisition(p2, posts=[post])
        assert np.all(x >= 0.0) and np.all(x <= 1.0) and np.isfinite(v)
    finally:
        post.close()
