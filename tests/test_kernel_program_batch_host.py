"""Host-side checks of the batched program-kernel entry points (no GPU): the header and the ctypes signatures of
boss_kgp_loglike_batch / boss_kgp_fit_batch, the refusals the library decides before it needs a device, S = 0, and the argument
handling of the two Python wrappers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nargs(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bosship.h")).read(), flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^;]*?)\);", hdr, re.S)
    assert m, name + " is not declared in include/bosship.h"
    return m.group(1).count(",") + 1


@pytest.fixture(scope="module")
def api():
    from boss_jl_amd import api
    api.load_library()
    return api


@pytest.fixture(scope="module")
def kern(api):
    k = api.KernelProgram(2, [1.0], [(api.FIT_OP["MUL"], 0, 2), (api.FIT_OP["MUL"], 1, 3), (api.FIT_OP["ADD"], 5, 6), (api.FIT_OP["ADD"], 7, 4)], 8)
    assert k.eval([0.5, 2.0], [3.0, 0.25]) == 0.5 * 3.0 + 2.0 * 0.25 + 1.0          # u·v + 1
    return k


def test_header_and_ctypes_signatures(api):
    for name, n in (("boss_kgp_loglike_batch", 15), ("boss_kgp_fit_batch", 16)):
        assert _nargs(name) == n, name
        res, args = api.SIGNATURES[name]
        assert res is C.c_int and len(args) == n, name
    ll, fit = api.SIGNATURES["boss_kgp_loglike_batch"][1], api.SIGNATURES["boss_kgp_fit_batch"][1]
    # (device, d, N, X, y, discrete, kern, S, lengthscales, amplitudes, noise_stds, mean_X, mean_stride, ll_out, status_out)
    assert ll[6] is C.c_void_p and ll[:3] == [C.c_int] * 3 and ll[7] is C.c_int and ll[12] is C.c_int and ll[14] == C.POINTER(C.c_int)
    # boss_gp_fit_batch's arguments with the program in the kernel id's place
    plain = api.SIGNATURES["boss_gp_fit_batch"][1]
    assert fit[1] is C.c_void_p and plain[1] is C.c_int and fit[:1] + fit[2:] == plain[:1] + plain[2:]
    jl = open(os.path.join(ROOT, "boss.jl_amd", "julia", "BOSSHip.jl")).read()
    for name in ("boss_kgp_loglike_batch", "boss_kgp_fit_batch"):
        assert re.search(r"# not bound: %s — .{10,}" % name, jl), name


def _arrays(api, d, N, S):
    rng = np.random.default_rng(0)
    X = api._f64(rng.uniform(0, 1, (d, N)), 2)
    y = api._f64(rng.standard_normal(N), 1)
    lam = api._f64(np.full((d, max(S, 1)), 0.5), 2)
    amp, sig = api._f64(np.ones(max(S, 1)), 1), api._f64(np.full(max(S, 1), 0.1), 1)
    return X, y, lam, amp, sig


def test_refusals_decided_before_a_device_is_needed(api, kern):
    """NULL kern, d != the program's x_dim, S < 0, NULL arrays with S > 0: BOSS_E_INVALID from both entry points on a machine
    without a GPU (the checks come before the device context is asked for); S = 0 returns BOSS_OK and writes nothing."""
    lib, dp = api.load_library(), api._dp
    d, N, S = 2, 7, 3
    X, y, lam, amp, sig = _arrays(api, d, N, S)
    ll = np.full(S, 7.0)
    st = np.full(S, 9, dtype=np.int32)
    stp = st.ctypes.data_as(C.POINTER(C.c_int))
    hs = (C.c_void_p * S)(*([12345] * S))

    def loglike(kern_h=kern._h, d_=d, S_=S, X_=X, y_=y, lam_=lam, amp_=amp, sig_=sig, out=ll):
        return lib.boss_kgp_loglike_batch(0, d_, N, dp(X_), dp(y_), None, kern_h, S_, dp(lam_), dp(amp_), dp(sig_), None, 0, dp(out), stp)

    def fit(kern_h=kern._h, d_=d, S_=S, X_=X, y_=y, lam_=lam, amp_=amp, sig_=sig, out=hs):
        return lib.boss_kgp_fit_batch(0, kern_h, d_, N, dp(X_), dp(y_), None, 0, None, S_, dp(lam_), dp(amp_), dp(sig_), out, dp(ll), stp)

    for call in (loglike, fit):
        for kw, msg in ((dict(kern_h=None), "kern is NULL"), (dict(d_=3), "x_dim = 2"), (dict(S_=-1), "S must be >= 0"),
                        (dict(X_=None), "non-NULL X, y"), (dict(y_=None), "non-NULL X, y"), (dict(lam_=None), "NULL hyper-parameter array"),
                        (dict(amp_=None), "NULL hyper-parameter array"), (dict(sig_=None), "NULL hyper-parameter array"),
                        (dict(out=None), "is NULL")):
            assert call(**kw) == api.BOSS_E_INVALID, (call.__name__, kw)
            assert msg in lib.boss_last_error().decode(), (call.__name__, kw, lib.boss_last_error().decode())
        assert call(S_=0) == api.BOSS_OK
        assert call(S_=0, lam_=None, amp_=None, sig_=None) == api.BOSS_OK
    assert np.all(ll == 7.0) and np.all(st == 9)             # nothing was written
    assert all(hs[s] is None for s in range(S))              # a refused fit leaves no handle behind


def test_python_wrappers_check_their_arguments(api, kern):
    d, N, S = 2, 7, 3
    X, y, lam, amp, sig = _arrays(api, d, N, S)
    for fn in (api.kgp_loglike_batch, api.kgp_fit_batch):
        with pytest.raises(TypeError, match="KernelProgram"):
            fn(X, y, "matern52", lam, amp, sig)
        with pytest.raises(api.BossError, match="d×S"):
            fn(X, y, kern, lam[:1], amp, sig)
        with pytest.raises(api.BossError, match="one entry per set"):
            fn(X, y, kern, lam, amp[:2], sig)
        with pytest.raises(ValueError, match="one entry per column"):
            fn(X, y[:-1], kern, lam, amp, sig)
        with pytest.raises(ValueError, match="S×N"):
            fn(X, y, kern, lam, amp, sig, mean_X=np.zeros((S + 1, N)))
        with pytest.raises(ValueError, match="S×N"):
            fn(X, y, kern, lam, amp, sig, mean_X=np.zeros(N + 1))
    with pytest.raises(api.BossError, match="finite"):
        api.kgp_fit_batch(X, y, kern, lam, [1.0, np.nan, 1.0], sig)
    # S = 0: empty results, no device
    ll, st = api.kgp_loglike_batch(X, y, kern, np.zeros((d, 0)), [], [])
    assert ll.shape == (0,) and st.shape == (0,)
    gps, ll, st = api.kgp_fit_batch(X, y, kern, np.zeros((d, 0)), [], [])
    assert gps == [] and ll.shape == (0,) and st.shape == (0,)
