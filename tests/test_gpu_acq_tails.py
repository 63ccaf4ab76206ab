"""GPU tests (pytest -m gpu) of the EI × feasibility epilogue (csrc/acq_kernels.hpp) in its tails, against 50-digit truths.

boss_acq_ei_moments and boss_acq_ei_grad_moments take the moments from the host, so ei_value, ei_accumulate_kernel,
acq_epilogue_kernel, ei_grad_point and ei_grad_kernel are driven with exactly chosen fp64 inputs and no GP.  The truths, their groups
and the bars come from tests/golden/acq_tails.json (generated on the CPU by tests/golden/make_acq_tails.py; no 50-digit arithmetic
runs here) and tests/acq_tails_cases.py:

    |got − truth| <= C·u·cond per candidate,  u = 2⁻⁵³,  cond the first-order condition sum of oracle/mp_oracle.acq_truth,
    C = 4 × the fp64 oracle's own worst err/(u·cond) over the fixture, rounded up to a power of two (the fixture's header).

Late in a BO run every candidate is worse than the incumbent: EI runs from 1e-20 down to 1e-300 and the arg-max is decided among
those values, which an absolute tolerance of 1e-10 does not see.  Every test prints err/(u·cond) per group; with
BOSS_ACQ_TAILS_REPORT=<file> the figures of test 1 are appended to that file as JSON lines (profiles/acq_tails.jsonl).

M <= 2100 per call; every test takes well under a second of device time."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import acq_tails_cases as A  # noqa: E402

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
POISON = -1.0000001e-8                       # just below −MAX_NEG_VAR


@pytest.fixture(scope="module")
def api():
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle
    return gp_oracle


@pytest.fixture(scope="module")
def fx():
    return A.load()


def report(rec):
    path = os.environ.get("BOSS_ACQ_TAILS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def check_argmax(acq, am, mx, what):
    """The returned max is acq[argmax] bit for bit, and argmax is the first index of the maximum (NaN largest)."""
    assert 0 <= am < acq.size, (what, am)
    assert same_bits(np.array([mx]), acq[am:am + 1]), f"{what}: max {mx!r} is not acq[{am}] = {acq[am]!r}"
    nan = np.isnan(acq)
    want = int(np.argmax(nan)) if nan.any() else int(np.argmax(acq))
    assert am == want, f"{what}: argmax {am}, first index of the maximum {want}"


# ------------------------------------------------------------------------------------------ 1. truths
def test_values_against_the_truths(api, fx):
    C = fx["header"]["device_C"]["value"]
    failures, by_decade = [], {}
    for g in fx["groups"]:
        if g["kind"] != "value":
            continue
        acq, am, mx = A.device_value(api, g)
        check_argmax(acq, am, mx, g["name"])
        if g["check"] == "tiny":
            print(f"{g['name']}: below 1e-280, device {acq.min():.3g} … {acq.max():.3g} (truth {g['truth'].min():.3g} … {g['truth'].max():.3g})")
            report({"group": g["name"], "check": "tiny", "device_min": float(acq.min()), "device_max": float(acq.max())})
            if not A.check_tiny(acq):
                failures.append(f"{g['name']}: not finite, >= 0 and <= {A.TINY_MAX:g}: {acq}")
            continue
        r = A.ratio(acq, g["truth"], g["cond"])
        bad = A.misses(acq, g["truth"], g["cond"], C)
        print(f"{g['name']}: P {g['P']} S {g['S']} M {g['M']} value err/(u·cond) = {r:.3g} (bar {C:g})")
        report({"group": g["name"], "P": g["P"], "S": g["S"], "M": g["M"], "value_ratio": r, "bar": C})
        if bad.any():
            j = int(np.argmax(bad))
            failures.append(f"{g['name']}: {int(bad.sum())} candidates outside the bar, first {j}: got {acq[j]!r}, truth {g['truth'][j]!r}, cond {g['cond'][j]:.3g}")
        # the arg-max is the truth's wherever the truth decides it
        bars = C * A.U * g["cond"]
        order = np.argsort(-g["truth"], kind="stable")
        if g["M"] >= 2 and np.isfinite(g["truth"][order[:2]]).all() and g["truth"][order[0]] - g["truth"][order[1]] > bars[order[0]] + bars[order[1]]:
            if am != order[0]:
                failures.append(f"{g['name']}: argmax {am}, the truth's {order[0]}")
        if g["name"].startswith("tail-"):
            pos = g["truth"] > 0
            if not np.all(acq[pos] > 0):
                failures.append(f"{g['name']}: acq <= 0 where the truth is representable and positive, at {np.flatnonzero(pos & ~(acq > 0))[:5].tolist()}")
            err, z = A.errors(acq, g["truth"]), A.z_of(g)
            for j in np.flatnonzero(g["cond"] > 0):
                k = A.decade(z[j])
                by_decade[k] = max(by_decade.get(k, 0.0), float(err[j] / (A.U * g["cond"][j])))
    print("tails, worst err/(u·cond) by decade of z: " + ", ".join(f"{k}: {v:.3g}" for k, v in sorted(by_decade.items())))
    report({"tails_by_z_decade": by_decade, "bar": C})
    assert not failures, "\n".join(failures)


def test_gradients_against_the_truths(api, fx):
    Cv, Cg = fx["header"]["device_C"]["value"], fx["header"]["device_C"]["grad"]
    failures = []
    for g in fx["groups"]:
        if g["kind"] != "grad":
            continue
        acq, dacq = A.device_grad(api, g)
        acq_v, _, _ = A.device_value(api, g)
        rv, rg = A.ratio(acq, g["truth"], g["cond"]), A.ratio(dacq, g["gtruth"], g["gcond"])
        print(f"{g['name']}: P {g['P']} d {g['d']} M {g['M']} err/(u·cond): value {rv:.3g} (bar {Cv:g}), gradient {rg:.3g} (bar {Cg:g})")
        report({"group": g["name"], "P": g["P"], "d": g["d"], "M": g["M"], "value_ratio": rv, "grad_ratio": rg, "bar": Cg})
        if not same_bits(acq, acq_v):
            failures.append(f"{g['name']}: the gradient call's value differs from acq_ei_moments' at {np.flatnonzero(acq != acq_v)[:5].tolist()}")
        if A.misses(acq, g["truth"], g["cond"], Cv).any():
            failures.append(f"{g['name']}: value outside the bar ({rv:.3g})")
        bad = A.misses(dacq, g["gtruth"], g["gcond"], Cg)
        if bad.any():
            k, j = np.argwhere(bad)[0]
            failures.append(f"{g['name']}: {int(bad.sum())} gradient entries outside the bar, first ∂{k} of {j}: got {dacq[k, j]!r}, truth {g['gtruth'][k, j]!r}, "
                            f"gcond {g['gcond'][k, j]:.3g}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------ 2. teeth on the device
def test_scaled_variances_miss_the_bar(api, fx):
    """The device given variances that are off by a factor 1 + 2⁻⁴⁰ against the unscaled truths: z moves by 4.5e-13 relative and EI by
    z²·4.5e-13, against a bar of 16·u·(1+z²)(|T1|+|T2|)/EI ≈ 2e-15·z⁴ relative — a miss for |z| up to about 15 wherever the bar's
    second term (P·Φ·(|μ|+|b|), the rounding of μf − b) is not what dominates it, which b = 0 guarantees.  Printed for every tail
    group, asserted for the six with b = 0."""
    C = fx["header"]["device_C"]["value"]
    scale = 1.0 + 2.0 ** -40
    for g in fx["groups"]:
        if not g["name"].startswith("tail-"):
            continue
        acq, _, _ = A.device_value(api, g, var_scale=scale)
        bad = A.misses(acq, g["truth"], g["cond"], C)
        print(f"{g['name']}: variances × (1 + 2⁻⁴⁰): {int(bad.sum())} of {g['M']} outside the bar, worst err/(u·cond) {A.ratio(acq, g['truth'], g['cond']):.3g}")
        if g["best"] == 0.0:
            assert bad.sum() >= 10, f"{g['name']}: a relative error of 2⁻⁴⁰ in σ² passes the bar"


# ------------------------------------------------------------------------------------------ 3. more than EI_MAXP outputs
YM16 = np.array([INF, 3.0, INF, INF, -0.5, INF, 40.0, INF, INF, INF, 2.5, INF, INF, 0.25, INF, 1e3])


@pytest.mark.parametrize("P", [17, 20])
def test_wide_outputs_are_their_16_output_twin(api, fx, P):
    """Above EI_MAXP = 16 the coefficients and constraints travel in device arrays: padded with outputs of coefficient 0 and
    y_max = +Inf, the call returns the bits of its 16-output twin — values and gradients, y_max present and NULL, S = 1 and 3."""
    g16 = fx["by_name"]["ei-p16"]
    assert same_bits(A.device_value(api, fx["by_name"][f"ei-p{P}"])[0], A.device_value(api, g16)[0])
    s3 = dict(g16, S=3, mu=np.concatenate([np.roll(g16["mu"], k, axis=2) for k in range(3)]), var=np.concatenate([np.roll(g16["var"], k, axis=2) for k in range(3)]))
    for base in (g16, s3):
        for ym in (None, YM16):
            b = dict(base, y_max=ym)
            for best in (b["best"], None):
                b2 = dict(b, best=best)
                a16, am16, mx16 = A.device_value(api, b2)
                aP, amP, mxP = A.device_value(api, A.pad_outputs(b2, P))
                what = f"P {P} S {b2['S']} y_max {'set' if ym is not None else 'NULL'} best {best}"
                assert same_bits(aP, a16) and amP == am16 and same_bits([mxP], [mx16]), what
                if best is not None:
                    assert np.all(np.isfinite(a16)) and a16.max() > 0, what
    gg = fx["by_name"]["g-ei-p16"]
    for ym in (None, YM16):
        b = dict(gg, y_max=ym)
        a16, d16 = A.device_grad(api, b)
        aP, dP = A.device_grad(api, A.pad_outputs(b, P))
        assert same_bits(aP, a16) and same_bits(dP, d16), f"gradient P {P} y_max {'set' if ym is not None else 'NULL'}"
        assert np.abs(d16).max() > 0
    assert same_bits(A.device_grad(api, fx["by_name"][f"g-ei-p{P}"])[1], A.device_grad(api, gg)[1])


# ------------------------------------------------------------------------------------------ 4. corners
def ei1(api, mu, var, best=1.5, y_max=None, mask=None, grads=None, coef=1.0):
    """P = 1 through both entry points: (acq[M], dacq[d, M]) with the values asserted bitwise equal."""
    mu, var = np.atleast_2d(np.asarray(mu, float)), np.atleast_2d(np.asarray(var, float))
    M = mu.shape[1]
    gm, gv = grads if grads is not None else (np.full((1, 2, M), 0.75), np.full((1, 2, M), -0.125))
    ym = None if y_max is None else [y_max]
    acq, am, mx = api.acq_ei_moments(mu, var, [coef], ym, best, mask)
    check_argmax(acq, am, mx, "corner")
    acq_g, dacq = api.acq_ei_grad_moments(mu, var, gm, gv, [coef], ym, best, mask)
    assert same_bits(acq, acq_g), (acq, acq_g)
    return acq, dacq


def test_corners_value_and_gradient(api):
    gm = np.array([[[0.75, 0.75, 0.75], [-2.0, -2.0, -2.0]]])             # ∇μ [1][d = 2][M = 3]
    gv = np.full((1, 2, 3), -0.125)
    # expected_improvement.jl:96-100 with σf = 0: diff == 0 → 0 (the explicit branch); diff > 0 → diff·Φ(+Inf) + 0·φ(+Inf) = diff, ∇ = ∇μf;
    # diff < 0 → diff·Φ(−Inf) + 0·φ(−Inf) = ∓0, ∇ = 0
    acq, dacq = ei1(api, [[1.5, 2.5, 0.5]], [[0.0, 0.0, 0.0]], grads=(gm, gv))
    assert acq[0] == 0.0 and acq[1] == 1.0 and acq[2] == 0.0, acq
    assert np.array_equal(dacq, [[0.0, 0.75, 0.0], [0.0, -2.0, 0.0]]), dacq
    # gaussian_process.jl:13 (MAX_NEG_VAR): var ∈ [−1e-8, 0) is 0
    mu = np.array([[1.5, 2.5, 0.5, 1.2, 3.0]])
    a0, d0 = ei1(api, mu, np.zeros((1, 5)))
    a1, d1 = ei1(api, mu, np.full((1, 5), -1e-9))
    assert same_bits(a0, a1) and same_bits(d0, d1)
    a0, d0 = ei1(api, mu, np.zeros((1, 5)), y_max=2.0)
    a1, d1 = ei1(api, mu, np.full((1, 5), -1e-9), y_max=2.0)
    assert same_bits(a0, a1) and same_bits(d0, d1)
    # acquisition.jl:21-25 (SafeFunction): var < −1e-8 → −Inf, ∇ = 0, in every mode but the constant one, for that candidate only
    mu, var = np.array([[1.0, 2.0, 3.0]]), np.array([[0.3, POISON, 0.3]])
    clean = np.array([[0.3, 0.3, 0.3]])
    for best, ym in ((1.5, None), (None, 2.5), (1.5, 2.5)):
        acq, dacq = ei1(api, mu, var, best=best, y_max=ym)
        ref, dref = ei1(api, mu, clean, best=best, y_max=ym)
        assert acq[1] == -INF and np.all(dacq[:, 1] == 0.0), (best, ym, acq, dacq)
        assert same_bits(acq[[0, 2]], ref[[0, 2]]) and same_bits(dacq[:, [0, 2]], dref[:, [0, 2]]) and np.all(np.isfinite(ref))
    # … and in the middle of an S = 3 sum (expected_improvement.jl:87-90): the mean is −Inf for that candidate only
    mu3 = np.array([[[1.0, 2.0, 3.0]], [[1.1, 2.1, 3.1]], [[0.9, 1.9, 2.9]]])
    var3 = np.array([clean, var, clean])
    acq, am, mx = api.acq_ei_moments(mu3, var3, [1.0], None, 1.5)
    ref, _, _ = api.acq_ei_moments(mu3, np.array([clean, clean, clean]), [1.0], None, 1.5)
    assert acq[1] == -INF and same_bits(acq[[0, 2]], ref[[0, 2]]) and am == 2 and mx == acq[2]
    # expected_improvement.jl:113-114 / StatsFuns.normcdf(μ, σ, x): σ == 0 and x == μ → 1;  y_max = −Inf → 0
    acq, dacq = ei1(api, [[0.7, 0.7]], [[0.0, 0.3]], best=None, y_max=0.7)
    assert acq[0] == 1.0 and acq[1] == 0.5 and np.all(dacq[:, 0] == 0.0), (acq, dacq)
    acq, dacq = ei1(api, [[0.7, -1e300, 0.7]], [[0.0, 0.3, 0.3]], best=None, y_max=-INF)
    assert np.all(acq == 0.0), acq
    acq, _ = ei1(api, [[2.0, 2.0]], [[0.3, 0.0]], best=1.5, y_max=-INF)
    assert np.all(acq == 0.0), acq
    # NaN moments: NaN for that candidate only, values and gradients
    for mu, var in (([[1.0, NAN, 3.0]], [[0.3, 0.3, 0.3]]), ([[1.0, 2.0, 3.0]], [[0.3, NAN, 0.3]])):
        acq, dacq = ei1(api, mu, var)
        ref, dref = ei1(api, [[1.0, 2.0, 3.0]], clean)
        assert np.isnan(acq[1]) and np.all(np.isnan(dacq[:, 1])), (acq, dacq)
        assert same_bits(acq[[0, 2]], ref[[0, 2]]) and same_bits(dacq[:, [0, 2]], dref[:, [0, 2]])
    # expected_improvement.jl:68-70: no incumbent and no constraints → acq ≡ 0, whatever the moments
    acq, dacq = ei1(api, [[1.0, NAN, 3.0, 2.0]], [[0.3, 0.3, POISON, NAN]], best=None, y_max=None)
    assert same_bits(acq, np.zeros(4)) and same_bits(dacq, np.zeros((2, 4))), (acq, dacq)
    # expected_improvement.jl:58-65 (make_safe): outside the domain acq = 0, ∇ = 0 — poisoned or NaN or not
    mask = np.array([True, False, False, False, True])
    acq, dacq = ei1(api, [[1.0, NAN, 3.0, 2.0, 2.0]], [[0.3, 0.3, POISON, 0.3, 0.3]], mask=mask)
    assert same_bits(acq[1:4], np.zeros(3)) and same_bits(dacq[:, 1:4], np.zeros((2, 3))) and acq[0] > 0 and acq[4] > acq[0], (acq, dacq)


# ------------------------------------------------------------------------------------------ 5. arg-max through acq_epilogue_kernel
def amax(api, vals, mask=None):
    """Candidates whose acquisition IS the given value: P = 1, coef 1, b = 0, σ² = 0 and μ = v > 0 give EI = v exactly (+Inf included);
    NaN: μ = NaN; −Inf: a poisoned variance.  S rows: the Bayesian-inference average."""
    v = np.atleast_2d(np.asarray(vals, dtype=np.float64))
    assert np.all((v > 0) | np.isnan(v) | np.isneginf(v))
    mu = np.where(np.isneginf(v), 1.0, v)[:, None, :]
    var = np.where(np.isneginf(v), -1.0, 0.0)[:, None, :]
    acq, am, mx = api.acq_ei_moments(mu, var, [1.0], None, 0.0, mask)
    assert same_bits([mx], acq[am:am + 1])
    return acq, am, mx


@pytest.mark.parametrize("M", [1, 2, 1023, 1024, 1025, 2049])
def test_argmax_sole_maximum(api, M):
    base = 1.0 + (np.arange(M) % 7) / 8.0
    for at in sorted({0, M - 1, 1023, 1024} & set(range(M))):
        v = base.copy()
        v[at] = 5.0
        acq, am, mx = amax(api, v)
        assert same_bits(acq, v) and am == at and mx == 5.0, (M, at, am, mx)


def test_argmax_ties_nan_and_poison(api):
    M = 2049
    base = 1.0 + (np.arange(M) % 7) / 8.0
    for pair in ((700, 1724), (1023, 1024), (5, 2048)):                    # same thread of the 1024-wide stride; neighbours; far apart
        v = base.copy()
        v[list(pair)] = 5.0
        assert amax(api, v)[1] == pair[0], pair
    v = base.copy()
    v[3], v[1500], v[476], v[1031] = INF, NAN, NAN, NAN                    # 476 = 1500 − 1024: one thread meets the later NaN … first
    acq, am, mx = amax(api, v)
    assert am == 476 and np.isnan(mx) and acq[3] == INF
    v = base.copy()
    v[2000], v[10] = NAN, INF
    assert amax(api, v)[1] == 2000, "NaN counts as the largest value (Julia argmax)"
    for m in (1, 1025, 2049):
        acq, am, mx = amax(api, np.full(m, -INF))
        assert am == 0 and mx == -INF and np.all(acq == -INF)
        v = base[:m].copy()
        v[m // 2] = NAN
        acq, am, mx = amax(api, v, mask=np.zeros(m, bool))
        assert am == 0 and same_bits([mx], [0.0]) and same_bits(acq, np.zeros(m))
    # S = 3: a tie that only the average creates ((1+2)+3 = (3+2)+1, each sample alone has another arg-max)
    v3 = np.tile(base[:1100] / 4.0, (3, 1))
    v3[:, 40], v3[:, 1090] = (3.0, 2.0, 1.0), (1.0, 2.0, 3.0)
    acq, am, mx = amax(api, v3)
    assert acq[40] == acq[1090] == mx and abs(mx - 2.0) < 1e-15 and am == 40
    assert [amax(api, v3[s])[1] for s in range(3)] == [40, 40, 1090]


# ------------------------------------------------------------------------------------------ 6. every handle path onto the same numbers
def far_setup(api, amp, N=1):
    """A posterior whose candidates are out of every training point's reach: K* is exactly 0 (sqexp at distance >= 1e6), so μ is the
    prior mean handed in, bit for bit, and σ² is whatever predict returns."""
    X = -1e6 - 100.0 * np.arange(N)[None, :]                              # training points out of each other's reach too
    g = api.GP(X, np.zeros(N), "sqexp")
    g.update([1.0], amp, 1.0)
    return g


def test_handle_paths_match_the_moments_path(api, O, fx):
    """boss_acq_ei (S = 1, 3; M = 1), boss_acq_ei_tracks, boss_acq_ei_grad, boss_acq_ei_grad_set and boss_gp_update_acq (small, and riding
    along the factorisation: rider_final_kernel / ei_value_one) against the moments entry points fed predict's moments, over
    z ∈ [−30, 5] at two amplitudes: within one bar of each other (printed: whether bitwise)."""
    C = max(fx["header"]["device_C"].values())
    M, best = 71, 1.7
    z = np.linspace(-30.0, 5.0, M)
    Xs = 1e6 + np.arange(M, dtype=np.float64)[None, :]
    cand = api.Candidates(Xs)
    rng = np.random.default_rng(5)
    mgrad = rng.standard_normal((1, M))
    seen = []

    def close(what, got, want, cond):
        bad = A.misses(got, want, cond, C)
        seen.append(what)
        print(f"{what}: {'bitwise' if same_bits(got, want) else f'err/(u·cond) {A.ratio(got, want, cond):.3g}'}")
        assert not bad.any(), f"{what}: outside one bar at {np.argwhere(bad)[:4].tolist()}"

    for amp in (1.0, 1e-3):
        mean = best + z * amp
        g = far_setup(api, amp)
        mu, var = g.predict(Xs, mean)
        assert same_bits(mu, mean) and np.all(var > 0)
        ref, am_ref, _ = api.acq_ei_moments(mu[None], var[None], [1.0], None, best)
        cond = A.ei_cond_fp64(O, mu, var, best)
        assert ref.min() > 0 and ref.min() < 1e-190, "the tail is reached"
        acq, am, mx = api.acq_ei([[g]], cand, [1.0], None, best, None, mean.reshape(1, 1, M))
        close(f"acq_ei α={amp:g}", acq, ref, cond)
        assert am == am_ref and mx == acq[am]
        for j in (0, 35):                                                  # the single-candidate call
            c1 = api.Candidates(Xs[:, j:j + 1])
            a1, am1, mx1 = api.acq_ei([[g]], c1, [1.0], None, best, None, mean[j:j + 1].reshape(1, 1, 1))
            close(f"acq_ei M=1 (candidate {j}) α={amp:g}", a1, ref[j:j + 1], cond[j:j + 1])
            assert am1 == 0 and mx1 == a1[0]
            c1.close()
        tr = api.Track(g, cand, mean)
        acq, am, _ = api.acq_ei_tracks([[tr]], [1.0], None, best)
        close(f"acq_ei_tracks α={amp:g}", acq, ref, cond)
        assert am == am_ref
        tr.close()
        # gradients
        mu_g, var_g, dmu, dvar = g.predict_grad(Xs, mean, mgrad)
        ref_a, ref_d = api.acq_ei_grad_moments(mu_g[None], var_g[None], dmu[None], dvar[None], [1.0], None, best)
        cond_g, gcond = A.ei_cond_fp64(O, mu_g, var_g, best, dmu, dvar)
        acq, dacq = api.acq_ei_grad([g], Xs, [1.0], None, best, None, mean[None], mgrad[None])
        close(f"acq_ei_grad value α={amp:g}", acq, ref_a, cond_g)
        close(f"acq_ei_grad gradient α={amp:g}", dacq, ref_d, gcond)
        assert np.abs(ref_d).max() > 0
        # S = 3: the handle and two more at nearby amplitudes, each with its own prior mean
        gs = [g, far_setup(api, amp * 1.25), far_setup(api, amp * 0.75)]
        means = np.array([mean, best + (z + 0.3) * amp, best + (z - 0.2) * amp])
        mv = [h.predict(Xs, m) for h, m in zip(gs, means)]
        mu3, var3 = np.array([t[0] for t in mv])[:, None, :], np.array([t[1] for t in mv])[:, None, :]
        ref3, am3, _ = api.acq_ei_moments(mu3, var3, [1.0], None, best)
        each = np.array([api.acq_ei_moments(mu3[s], var3[s], [1.0], None, best)[0] for s in range(3)])
        cond3 = A.mean_cond(np.array([A.ei_cond_fp64(O, mu3[s, 0], var3[s, 0], best) for s in range(3)]), each)
        acq, am, _ = api.acq_ei([[h] for h in gs], cand, [1.0], None, best, None, means.reshape(3, 1, M))
        close(f"acq_ei S=3 α={amp:g}", acq, ref3, cond3)
        assert am == am3
        pg = [h.predict_grad(Xs, m, mgrad) for h, m in zip(gs, means)]
        parts = [api.acq_ei_grad_moments(t[0][None], t[1][None], t[2][None], t[3][None], [1.0], None, best) for t in pg]
        gc = [A.ei_cond_fp64(O, t[0], t[1], best, t[2], t[3]) for t in pg]
        want_a, want_d = np.mean([p[0] for p in parts], axis=0), np.mean([p[1] for p in parts], axis=0)
        acq, dacq = api.acq_ei_grad_set([[h] for h in gs], Xs, [1.0], None, best, None, means.reshape(3, 1, M), np.tile(mgrad, (3, 1, 1, 1)).reshape(3, 1, 1, M))
        close(f"acq_ei_grad_set value α={amp:g}", acq, want_a, A.mean_cond(np.array([t[0] for t in gc]), np.array([p[0] for p in parts])))
        close(f"acq_ei_grad_set gradient α={amp:g}", dacq, want_d, A.mean_cond(np.array([t[1] for t in gc]), np.array([p[1] for p in parts])))
        for h in gs:
            h.close()
        # boss_gp_update_acq: N <= 128 (the two phases one after the other) and N = 300, the smallest size at which
        # tests/test_gpu_rider.py sees the substitution ride along: rider_final_kernel answers
        for N, fused in ((1, False), (300, True)):
            h = far_setup(api, amp, N)
            r = h.update_acq([1.0], amp, 1.0, cand, best=best, mean_Xs=mean, want_acq=True, want_moments=True)
            assert r["fused"] == fused, (N, r["fused"], api._fallbacks(0))
            assert same_bits(r["mu"], mean)
            want, am_w, _ = api.acq_ei_moments(r["mu"][None], r["var"][None], [1.0], None, best)
            close(f"update_acq N={N} (fused {r['fused']}) α={amp:g}", r["acq"], want, A.ei_cond_fp64(O, r["mu"], r["var"], best))
            assert r["argmax"] == am_w and r["max"] == r["acq"][r["argmax"]] and r["acq"].min() > 0
            h.close()
    cand.close()
    assert len(seen) == 2 * 11
