"""GPU tests (pytest -m gpu) of the device's accuracy over the hyper-parameter range, against 50-digit truths.

The truths, their grid and the bars come from tests/golden/regimes.json (generated on the CPU by tests/golden/make_regimes.py; no
50-digit arithmetic runs here) and tests/regimes_cases.py: λ from 0.01·√d to 30·√d, α from 0.05 to 30, σ from 1e-3 to 2 for the
plain GP; the gradient-observation and the Gibbs model over their own grids.  With B = cond(K)·rows·u, u = 2⁻⁵³:

    logpdf  8·B·(1 + |ℓ|)     μ  8·B·(1 + max|μ|)     var  8·B·α²     every gradient  100·B·(1 + max|want|)

— the project's bars without the 1e-9 floor, against a truth that has no rounding of its own.  Every test prints err/(B·scale) per
case and quantity (the bars are 8 and 100 in that unit).  Candidates whose true variance is within 2 bars + 1e-8 of zero are left out
of the prediction calls (the device clips there; regimes_cases.keep_mask).  A BOSS_E_NOT_PD or BOSS_E_NEG_VAR fails the test: the
50-digit factorisation of every case in the fixture succeeds.

Shapes: (d, N, M) = (2, 40, 6) and (3, 136, 9) for the plain GP (one workgroup; one block past 128, the blocked factor and
predict_kernel), n = 12 and 45 points (36 and 135 rows) for the gradient model, N = 40 and 136 for the Gibbs model."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import regimes_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [("plain", "a"), ("plain", "b"), ("grad", "n12"), ("grad", "n45"), ("gibbs", "n40"), ("gibbs", "n136")]


@pytest.fixture(scope="module")
def api():
    import __graft_entry__ as entry
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def fx():
    return R.load()


def cases(fx, model, data):
    return [c for c in fx[model]["cases"] if c["data"] == data]


def new_handle(api, fx, model, c):
    D = fx[model]["datasets"][c["data"]]
    if model == "plain":
        return api.GP(D["X"], D["y"], c["kernel"])
    if model == "grad":
        return api.GradGP(D["X"], D["y"], D["dY"], c["kernel"])
    return api.GibbsGP(D["X"], D["y"])


def fmt(r):
    return " ".join(f"{k} {v:.3g}" for k, v in r.items())


# ------------------------------------------------------------------------------------------ 1. the handles against the truths
@pytest.mark.parametrize("model,data", SIZES)
def test_handles_against_the_truths(api, fx, model, data):
    """GP / GradGP / GibbsGP: update, predict, predict_grad (plain), loglike_grad in every regime of the grid, one resident handle per
    kernel re-fitted from regime to regime as a fitter does."""
    handles, failures = {}, []
    try:
        for c in cases(fx, model, data):
            key = c.get("kernel")
            if key not in handles:
                handles[key] = new_handle(api, fx, model, c)
            for what, got, keep in R.DEVICE[model](api, fx, c, handles[key]):
                r = R.ratios(c, got, model, keep)
                print(f"{c['name']} cond {c['cond']:.3g} kept {int(keep.sum())}/{keep.size} {what}: {fmt(r)}")
                try:
                    R.check(c, got, model, what, keep=keep)
                except AssertionError as e:
                    failures.append(str(e))
    finally:
        for h in handles.values():
            h.close()
    assert not failures, f"{len(failures)} misses:\n" + "\n".join(failures[:40])


@pytest.mark.parametrize("shift", [-1e-8, 1e-8])
@pytest.mark.parametrize("model", ["plain", "grad", "gibbs"])
def test_a_lift_error_on_the_device_would_be_caught(api, fx, model, shift):
    """The comparison above has teeth on the device's own results: handed parameters that are off by ∓1e-8 (what a +1e-8 lift left out
    or applied twice on one path amounts to), the device misses a bar in at least one of the best-conditioned cases of each model."""
    caught = None
    for c in sorted(fx[model]["cases"], key=R.unit)[:10]:
        for what, got, keep in R.DEVICE[model](api, fx, c, None, shift):
            out = {k: v for k, v in R.ratios(c, got, model, keep).items() if v > R.LIMIT[k]}
            if out and caught is None:
                caught = (c["name"], what, out)
    print(model, shift, "caught by", caught)
    assert caught is not None


# ------------------------------------------------------------------------------------------ 2. the batch twins in the same regimes
def handle_results(api, fx, model, cs):
    """(logpdf[S], llgrad[..., S]) of the single-handle path, one fresh update per case."""
    lps, grads = [], []
    h = new_handle(api, fx, model, cs[0])
    try:
        for c in cs:
            out = R.DEVICE[model](api, fx, c, h)
            lps.append(out[0][1]["logpdf"])
            assert out[1][1]["logpdf"] == lps[-1]
            grads.append(out[1][1]["llgrad"])
    finally:
        h.close()
    return np.array(lps), np.stack(grads, axis=-1)


@pytest.mark.parametrize("data", ["a", "b"])
@pytest.mark.parametrize("kernel", R.KERNELS)
def test_plain_batches_over_all_regimes(api, fx, kernel, data):
    """loglike_batch and loglike_grad_batch_mean with every regime of a kernel as one batch of S sets (a third of the sets with their
    prior mean, the others with a zero row).  Against the truths by the bars; against the handle results by the bounds the suite already
    holds between the two paths wherever those bounds are the larger of the two (tests/test_gpu_parity.py: 1e-11·(1 + |ℓ|) on the
    likelihood, 1e-10·(1 + max|g|) on the gradient) and by the truth bars elsewhere — in the ill-conditioned regimes two schedules of
    the same factorisation differ by a multiple of cond·u, which a fixed bound cannot hold."""
    cs = [c for c in cases(fx, "plain", data) if c["kernel"] == kernel]
    S = len(cs)
    inp = [R.plain_inputs(fx, c) for c in cs]
    X, y = inp[0][0], inp[0][1]
    lam = np.asfortranarray(np.stack([i[3] for i in inp], axis=1))
    amp, sig = np.array([i[4] for i in inp]), np.array([i[5] for i in inp])
    means = np.stack([np.zeros(X.shape[1]) if i[6] is None else i[6] for i in inp])
    lp_h, gr_h = handle_results(api, fx, "plain", cs)
    ll, st = api.loglike_batch(X, y, kernel, lam, amp, sig, mean_X=means)
    ll_g, st_g, gr = api.loglike_batch(X, y, kernel, lam, amp, sig, mean_X=means, want_grad=True)
    ll_m, st_m, gr_m, dmean, _ = api.loglike_grad_batch_mean(X, y, kernel, lam, amp, sig, mean_X=means, want_dmean=True)
    assert not st.any() and not st_g.any() and not st_m.any(), (st, st_g, st_m)
    assert np.array_equal(ll_g, ll_m) and np.array_equal(gr, gr_m)
    failures = []
    for s, c in enumerate(cs):
        for what, got in (("loglike_batch", {"logpdf": ll[s]}), ("loglike_grad_batch_mean", {"logpdf": ll_m[s], "llgrad": gr_m[:, s]})):
            print(f"{c['name']} cond {c['cond']:.3g} {what}: {fmt(R.ratios(c, got, 'plain'))}")
            try:
                R.check(c, got, "plain", what)
            except AssertionError as e:
                failures.append(str(e))
        d_ll = max(abs(ll[s] - lp_h[s]), abs(ll_m[s] - lp_h[s]))
        d_gr = np.abs(gr_m[:, s] - gr_h[:, s]).max()
        b_ll = max(1e-11 * (1 + abs(lp_h[s])), R.bar_logpdf(c, c["logpdf"]))
        b_gr = max(1e-10 * (1 + np.abs(gr_h[:, s]).max()), R.bar_grad(c, c["llgrad"]))
        print(f"    batch − handle: ll {d_ll:.3g} (bound {b_ll:.3g}) grad {d_gr:.3g} (bound {b_gr:.3g})")
        if d_ll > b_ll or d_gr > b_gr:
            failures.append(f"{c['name']}: batch − handle ll {d_ll:.3g} > {b_ll:.3g} or grad {d_gr:.3g} > {b_gr:.3g}")
    assert np.isfinite(dmean).all()
    assert not failures, f"{len(failures)} misses:\n" + "\n".join(failures[:40])


@pytest.mark.parametrize("data", ["n12", "n45"])
@pytest.mark.parametrize("kernel", R.KERNELS)
def test_gradient_model_batches_equal_the_handles_bitwise(api, fx, kernel, data):
    """ggp_loglike_batch / ggp_loglike_grad_batch over all regimes of a kernel as one batch: the bits of GradGP.update + loglike_grad
    (as tests/test_gpu_model_llgrad_batch.py holds in the tame regime), hence within the truth bars by test 1."""
    cs = [c for c in cases(fx, "grad", data) if c["kernel"] == kernel]
    inp = [R.grad_inputs(fx, c) for c in cs]
    X, y, dY = inp[0][:3]
    lam = np.asfortranarray(np.stack([i[4] for i in inp], axis=1))
    amp, sig, sgd = (np.array([i[k] for i in inp]) for k in (5, 6, 7))
    lp_h, gr_h = handle_results(api, fx, "grad", cs)
    ll, st = api.ggp_loglike_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    ll_g, st_g, gr = api.ggp_loglike_grad_batch(X, y, dY, kernel, lam, amp, sig, sgd)
    print(f"{data} {kernel}: max |ll − handle| {np.abs(ll - lp_h).max():.3g} max |grad − handle| {np.abs(gr - gr_h).max():.3g}")
    assert not st.any() and not st_g.any()
    assert np.array_equal(ll, lp_h) and np.array_equal(ll_g, lp_h) and np.array_equal(gr, gr_h)


@pytest.mark.parametrize("data", ["n40", "n136"])
def test_gibbs_batches_equal_the_handles_bitwise(api, fx, data):
    """ngp_loglike_batch / ngp_loglike_grad_batch over all regimes of a size as one batch: the bits of GibbsGP.update + loglike_grad."""
    cs = cases(fx, "gibbs", data)
    inp = [R.gibbs_inputs(fx, c) for c in cs]
    X, y = inp[0][0], inp[0][1]
    lam = np.asfortranarray(np.stack([i[3] for i in inp], axis=2))
    amp, noi = (np.asfortranarray(np.stack([i[k] for i in inp], axis=1)) for k in (4, 5))
    lp_h, gr_h = handle_results(api, fx, "gibbs", cs)
    ll, st = api.ngp_loglike_batch(X, y, lam, amp, noi)
    ll_g, st_g, dlam, damp, dnoise, _ = api.ngp_loglike_grad_batch(X, y, lam, amp, noi)
    gr = np.concatenate([dlam, damp[None], dnoise[None]], axis=0)
    print(f"{data}: max |ll − handle| {np.abs(ll - lp_h).max():.3g} max |grad − handle| {np.abs(gr - gr_h).max():.3g}")
    assert not st.any() and not st_g.any()
    assert np.array_equal(ll, lp_h) and np.array_equal(ll_g, lp_h) and np.array_equal(gr, gr_h)


# ------------------------------------------------------------------------------------------ 3. append in the regimes
@pytest.mark.parametrize("model", ["plain", "grad", "gibbs"])
def test_append_in_the_regimes(api, fx, model):
    """The corner subset (regimes_cases.is_corner): a handle fitted on the first N − 5 points, the last 5 appended in one block and, on a
    second handle, one by one; logpdf and one prediction against the truth of the N-point case, by the same bars.  An append that
    rebuilds its parameters only "up to rounding" (1/invλ − 1e-8 for λ) is off by 1e-8·|∂/∂λ| here and misses the bars of the
    well-conditioned cases."""
    failures = []
    for c in fx[model]["cases"]:
        if not R.is_corner(model, c):
            continue
        for one_by_one in (False, True):
            what = "append one by one" if one_by_one else "append block"
            got, keep = R.device_append(api, model, fx, c, one_by_one)
            print(f"{c['name']} cond {c['cond']:.3g} {what}: {fmt(R.ratios(c, got, model, keep))}")
            try:
                R.check(c, got, model, what, keep=keep)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, f"{len(failures)} misses:\n" + "\n".join(failures[:40])
