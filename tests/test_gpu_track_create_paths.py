"""The one track-create path of the three models (track_create, csrc/host_track.inc): a failed device allocation leaves nothing
behind and nothing broken, a deferred update is finished under the lock instead of being refused, and a handle that was never
updated is refused.

Shapes: 40 rows (the gradient model: 10 points, d = 3) and 33 candidates — two candidate tiles, the second partial.  Bounds: moments
of two tracks built by the same launches on the same data are compared bit for bit; `predict` runs another kernel than the track's
rebuild at this size (the one-workgroup path), so the two agree to rounding only: 1e-12 absolute on moments of order 1 (cond(K) is
below 1e3 here: σ = 0.1 on α = 1)."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
D, ROWS, M = 3, 40, 33
MODELS = ["plain", "gibbs", "grad"]


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


class Case:
    """One model's data, a fitted (or not yet updated) handle of it, its track and its one-shot prediction at the candidates."""

    def __init__(self, model):
        self.model = model
        rng = np.random.default_rng(11)
        n = ROWS // (1 + D) if model == "grad" else ROWS
        self.X = rng.uniform(0, 1, (D, n))
        w = np.linspace(1.0, 2.0, D)[:, None]
        self.y = np.sin(2 * np.pi * w * self.X).sum(0)
        self.dY = 2 * np.pi * w * np.cos(2 * np.pi * w * self.X)
        self.Xs = np.asfortranarray(rng.uniform(0, 1, (D, M)))
        self.lam = np.linspace(0.4, 0.6, D)

    def latent(self, P):
        """λ(x) d×n, α(x) n, σ(x) n of the nonstationary model at the points P"""
        lam = self.lam[:, None] * (1.0 + 0.3 * P)
        return np.asfortranarray(lam), 1.0 + 0.2 * P[0], 0.1 + 0.02 * P[1]

    def handle(self, api):
        if self.model == "grad":
            return api.GradGP(self.X, self.y, self.dY, "matern52")
        if self.model == "gibbs":
            return api.GibbsGP(self.X, self.y)
        return api.GP(self.X, self.y, "matern52")

    def update(self, g, sync=True):
        if self.model == "grad":
            return g.update(self.lam, 1.0, 0.1, 0.1, sync=sync)
        if self.model == "gibbs":
            return g.update(*self.latent(self.X), sync=sync)
        return g.update(self.lam, 1.0, 0.1, sync=sync)

    def track(self, api, g, cand):
        if self.model == "grad":
            return api.GradTrack(g, cand)
        if self.model == "gibbs":
            lam, amp, _ = self.latent(self.Xs)
            return api.GibbsTrack(g, cand, lam, amp)
        return api.Track(g, cand)

    def predict(self, g):
        if self.model == "gibbs":
            lam, amp, _ = self.latent(self.Xs)
            return g.predict(self.Xs, lam, amp)
        return g.predict(self.Xs)


def drop_parked_slab(api):
    """Storage a released batch-fitted set left with the context would absorb a simulated failure (dev_malloc drops it and tries
    again): give it back first, as tests/test_gpu_fit_batch.py does, so that the next failure surfaces."""
    lib = api.load_library()
    lib.boss_debug_slab_cache_bytes.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
    nbytes = C.c_size_t(0)
    lib.boss_debug_slab_cache_bytes(0, C.byref(nbytes))
    if nbytes.value:
        lib.boss_debug_fail_next_alloc(1)
        api.GP(np.zeros((1, 2)), np.zeros(2)).close()              # its first allocation "fails": the parked block goes
        lib.boss_debug_fail_next_alloc(0)
        lib.boss_debug_slab_cache_bytes(0, C.byref(nbytes))
        assert nbytes.value == 0


@pytest.mark.parametrize("model", MODELS)
def test_failed_allocation_leaves_nothing_broken(api, model):
    lib = api.load_library()
    case = Case(model)
    g = case.handle(api)
    case.update(g)
    cand = api.Candidates(case.Xs)
    ref = case.track(api, g, cand)                                 # (the shared workspaces have their sizes from here on)
    mu_r, var_r = ref.moments()
    drop_parked_slab(api)
    lib.boss_debug_fail_next_alloc(1)
    try:
        with pytest.raises(api.BossError) as e:
            case.track(api, g, cand)
    finally:
        lib.boss_debug_fail_next_alloc(0)
    assert e.value.code == api.BOSS_E_ALLOC
    tr = case.track(api, g, cand)
    mu, var = tr.moments()
    assert np.array_equal(mu, mu_r) and np.array_equal(var, var_r)
    mu_p, var_p = case.predict(g)
    err = (np.abs(mu_p - mu_r).max(), np.abs(var_p - np.maximum(var_r, 0.0)).max())
    print(f"{model}: predict against the reference track: mu {err[0]:.2e}  var {err[1]:.2e}", flush=True)
    assert err[0] <= 1e-12 and err[1] <= 1e-12, err
    for t in (tr, ref):
        t.close()
    cand.close()
    g.close()


def test_deferred_update_is_settled_not_refused(api):
    case = Case("plain")
    cand = api.Candidates(case.Xs)
    g1, g2 = case.handle(api), case.handle(api)
    assert case.update(g1, sync=False) is None
    t1 = api.Track(g1, cand)                                       # at once: the update is finished under the lock
    case.update(g2, sync=False)
    g2.sync()
    t2 = api.Track(g2, cand)
    (mu1, var1), (mu2, var2) = t1.moments(), t2.moments()
    assert np.isfinite(mu1).all() and np.isfinite(var1).all()
    assert np.array_equal(mu1, mu2) and np.array_equal(var1, var2)
    for o in (t1, t2, cand, g1, g2):
        o.close()


@pytest.mark.parametrize("model", MODELS)
def test_never_updated_handle_is_refused(api, model):
    case = Case(model)
    g = case.handle(api)
    cand = api.Candidates(case.Xs)
    with pytest.raises(api.BossError) as e:
        case.track(api, g, cand)
    assert e.value.code == api.BOSS_E_NOT_FITTED
    case.update(g)
    case.track(api, g, cand).close()                               # the same handle, fitted: accepted
    cand.close()
    g.close()
