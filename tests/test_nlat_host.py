"""Resident latent models of a NonstationaryGP, the parts that need no device: declarations, bindings, the Julia glue, device_spec,
argument checks, and the closed forms of the transforms against the host path (scipy's ppf(ndtr(m)))."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("boss_nlat_create", "boss_nlat_free", "boss_nlat_eval", "boss_ngp_predict_lat", "boss_ngp_predict_grad_lat",
       "boss_ngp_predict_set_lat", "boss_ngp_predict_grad_set_lat", "boss_ngp_acq_ei_grad_set_lat")


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    return a


@pytest.fixture(scope="module")
def B(api):
    import boss_jl_amd
    return boss_jl_amd


def test_symbols_are_declared_exported_and_bound(api):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bosship.h")).read(), flags=re.S)
    lib = api.load_library()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name + " is not declared in include/bosship.h"
        assert hasattr(lib, name), name + " is not exported"
        assert name in api.SIGNATURES, name + " is not bound in api.py"
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\);", hdr, re.S).group(1)
        assert len(api.SIGNATURES[name][1]) == decl.count(",") + 1, name
    for code, val in (("BOSS_LT_NONE", 0), ("BOSS_LT_NORMAL", 1), ("BOSS_LT_LOGNORMAL", 2), ("BOSS_LT_UNIFORM", 3),
                      ("BOSS_ACT_IDENTITY", 0), ("BOSS_ACT_SOFTPLUS", 1), ("BOSS_ACT_EXP", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (code, val), hdr), code
    assert api.LATENT_TARGETS == {"none": 0, "normal": 1, "lognormal": 2, "uniform": 3}
    assert api.LATENT_ACTS == {"identity": 0, "softplus": 1, "exp": 2}
    for name in ("NgpLatents", "ngp_predict_set_lat", "ngp_predict_grad_set_lat", "ngp_acq_ei_grad_set_lat"):
        assert hasattr(api, name), name
    assert hasattr(api.GibbsGP, "predict_lat") and hasattr(api.GibbsGP, "predict_grad_lat")


def test_public_names_are_exported(B):
    for name in ("NgpLatents", "ngp_predict_set_lat", "ngp_predict_grad_set_lat", "ngp_acq_ei_grad_set_lat", "identity_act", "softplus",
                 "exp_act", "constant_latent", "latent_transform", "LatentActivation"):
        assert hasattr(B, name), name


def test_julia_glue_binds_the_calls_and_the_document_mirrors_it():
    jl = open(os.path.join(ROOT, "boss.jl_amd", "julia", "BOSSHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert jl in doc
    called = set(re.findall(r"\(:(boss_[a-z0-9_]+), lib\)", jl))
    for name in NEW:
        assert name in called, name + " has no ccall in BOSSHip.jl"
    assert "mutable struct HipLatents" in jl and re.search(r"function HipLatents\(", jl)
    for word in ("ParametrizedGP", "ParametrizedGPParams", "Normal", "LogNormal", "Uniform", "softplus", "identity", "exp"):
        assert word in jl[jl.index("mutable struct HipLatents"):], word


def test_device_spec_recognises_the_closed_family(B):
    from scipy import stats
    P = B.HipParametrizedGP
    assert P([1.0]).device_spec() == ("none", (0.0, 0.0), "identity", 0.0)
    assert P([1.0], target_dist=stats.norm(1.0, 0.3), act_func=B.identity_act).device_spec() == ("normal", (1.0, 0.3), "identity", 0.0)
    t, (p0, p1), a, ap = P([1.0], target_dist=stats.lognorm(0.5, scale=np.exp(-0.7)), act_func=B.softplus).device_spec()
    assert (t, a, ap) == ("lognormal", "softplus", 0.0) and abs(p0 + 0.7) < 1e-15 and p1 == 0.5
    assert P([1.0], target_dist=stats.uniform(0.2, 1.8), act_func=B.exp_act).device_spec() == ("uniform", (0.2, 2.0), "exp", 0.0)
    assert P([1.0], act_func=B.softplus.with_lower_bound(0.1)).device_spec() == ("none", (0.0, 0.0), "softplus", 0.1)
    # outside the family
    assert P([1.0], target_dist=stats.gamma(2.0), act_func=B.identity_act).device_spec() is None
    assert P([1.0], target_dist=stats.lognorm(0.5, loc=0.1), act_func=B.identity_act).device_spec() is None
    assert P([1.0], act_func=lambda z: z).device_spec() is None
    # the activation objects are ordinary array functions
    z = np.array([-800.0, -1.0, 0.0, 2.0, 800.0])
    assert np.array_equal(B.identity_act(z), z) and np.allclose(B.exp_act(z[1:4]), np.exp(z[1:4]))
    sp = B.softplus.with_lower_bound(0.1)(z)
    assert np.all(np.isfinite(sp)) and sp[0] == 0.1 and sp[4] == 800.1 and abs(sp[2] - (np.log(2.0) + 0.1)) < 1e-15


def test_resident_latents_with_an_indescribable_latent_raises(B):
    from scipy import stats
    const = B.constant_latent(0.5)
    ok = B.HipNonstationaryGP([B.stack_latents([const, const])], [const], [const], resident_latents=True)
    assert ok.resident_latents
    with pytest.raises(ValueError, match=r"f_amp\[0\]"):
        B.HipNonstationaryGP([B.stack_latents([const, const])], [lambda x: 1.0], [const], resident_latents=True)
    with pytest.raises(ValueError, match=r"f_lam\[0\]\[1\]"):
        B.HipNonstationaryGP([B.stack_latents([const, lambda x: 1.0])], [const], [const], resident_latents=True)
    with pytest.raises(ValueError, match=r"f_lam\[0\]"):
        B.HipNonstationaryGP([lambda x: np.ones(2)], [const], [const], resident_latents=True)

    def fake_post(model):                                        # a posterior closure as model_posterior returns it, without a device
        f = lambda x: 1.0                                        # noqa: E731
        f.model, f.gp = model, object()
        return f
    bad = fake_post(B.HipParametrizedGP([1.0, 1.0], target_dist=stats.gamma(2.0), act_func=B.identity_act))
    with pytest.raises(ValueError, match=r"f_lam\[0\]\[0\].*not one the device evaluates"):
        B.HipNonstationaryGP([B.stack_latents([bad, const])], [const], [const], resident_latents=True)
    # the default leaves everything as it was
    plain = B.HipNonstationaryGP([lambda x: np.ones(2)], [lambda x: 1.0], [lambda x: 0.1])
    assert plain.resident_latents is False


def _create(api, d, lam_const, amp_const=1.0, noise_const=float("nan"), out=True):
    lib = api.load_library()
    nq = d + 2
    handles = (C.c_void_p * max(d, 1))()
    lam = np.asarray(lam_const, float)
    tgt, act = (C.c_int * nq)(), (C.c_int * nq)()
    tpar, apar = np.zeros(2 * nq), np.zeros(nq)
    h = C.c_void_p()
    return lib.boss_nlat_create(0, d, handles, api._dp(lam), None, amp_const, None, noise_const, tgt, api._dp(tpar), act, api._dp(apar), None,
                                C.byref(h) if out else None)


def test_argument_checks_need_no_device(api):
    assert _create(api, 17, np.ones(17)) == api.BOSS_E_INVALID                    # d > 16
    assert _create(api, 0, np.ones(1)) == api.BOSS_E_INVALID
    assert _create(api, 2, np.ones(2), out=False) == api.BOSS_E_INVALID           # NULL output pointer
    assert _create(api, 2, [1.0, np.inf]) == api.BOSS_E_INVALID                   # a NULL latent with a non-finite constant
    assert _create(api, 2, [1.0, np.nan]) == api.BOSS_E_INVALID
    assert _create(api, 2, np.ones(2), amp_const=np.nan) == api.BOSS_E_INVALID
    assert _create(api, 2, np.ones(2), noise_const=np.inf) == api.BOSS_E_INVALID  # (NaN = no noise model, Inf is not a constant)
    lib = api.load_library()
    z = np.zeros(4)
    bad = C.c_long(0)
    assert lib.boss_nlat_eval(None, 1, api._dp(z), api._dp(z), api._dp(z), None, None, None, C.byref(bad)) == api.BOSS_E_INVALID
    assert lib.boss_ngp_predict_lat(None, 1, api._dp(z), None, None, api._dp(z), api._dp(z), C.byref(bad)) == api.BOSS_E_INVALID
    assert lib.boss_ngp_predict_grad_lat(None, 1, api._dp(z), None, None, None, api._dp(z), api._dp(z), api._dp(z), api._dp(z),
                                         C.byref(bad)) == api.BOSS_E_INVALID
    assert lib.boss_ngp_predict_set_lat(1, None, 1, api._dp(z), None, None, api._dp(z), api._dp(z), C.byref(bad)) == api.BOSS_E_INVALID
    assert lib.boss_ngp_predict_grad_set_lat(0, None, 1, api._dp(z), None, None, None, api._dp(z), api._dp(z), api._dp(z), api._dp(z),
                                             C.byref(bad)) == api.BOSS_E_INVALID
    assert lib.boss_ngp_acq_ei_grad_set_lat(1, 1, None, 1, api._dp(z), None, None, None, api._dp(z), None, 0, 0.0, None, api._dp(z),
                                            api._dp(z)) == api.BOSS_E_INVALID
    lib.boss_nlat_free(None)                                                      # a no-op


def test_without_a_device_create_fails_loudly(api):
    import torch
    if torch.cuda.is_available():
        assert api.device_count() >= 1                                            # (the device tests cover the rest)
        return
    assert _create(api, 2, np.ones(2)) == api.BOSS_E_NO_DEVICE
    assert _create(api, 2, np.ones(2), noise_const=0.1) == api.BOSS_E_NO_DEVICE
    with pytest.raises(api.BossError) as e:
        api.NgpLatents([0.5, 0.5], 1.0)
    assert e.value.code == api.BOSS_E_NO_DEVICE


def test_a_closed_latent_handle_is_named(api):
    """A closed GP handle must not reach the library as NULL, where it would mean "the constant beside it"."""
    class Closed:
        _h = None
    spec = ("none", (0.0, 0.0), "identity", 0.0)
    for lam, amp, noise, name in [([0.5, (Closed(), spec)], 1.0, None, "lengthscale latent 1"), ([0.5, 0.5], (Closed(), spec), None, "amplitude"),
                                  ([0.5, 0.5], 1.0, (Closed(), spec), "noise")]:
        with pytest.raises(api.BossError, match=name + ".*closed") as e:
            api.NgpLatents(lam, amp, noise)
        assert e.value.code == api.BOSS_E_INVALID


# ------------------------------------------------------------------------------------------ closed forms against the host path
M_GRID = np.linspace(-3.0, 3.0, 2001)


def _dists():
    from scipy import stats
    return {"lognormal": stats.lognorm(0.5, scale=np.exp(-0.7)), "normal": stats.norm(1.0, 0.3), "uniform": stats.uniform(0.2, 1.8), "none": None}


@pytest.mark.parametrize("target", ["lognormal", "normal", "uniform", "none"])
def test_closed_forms_agree_with_the_host_transform(B, target):
    """HipParametrizedGP.transform (ppf(ndtr(m))) against the closed form on m in [-3, 3]: 1e-13 relative (measured with scipy 1.15.3:
    5.8e-15 LogNormal(-0.7, 0.5), 3.1e-15 Normal(1, 0.3), 0 Uniform — the bound leaves ≈ 17×)."""
    for act in (B.identity_act, B.softplus.with_lower_bound(0.1), B.exp_act):
        pg = B.HipParametrizedGP([1.0], target_dist=_dists()[target], act_func=act)
        spec = pg.device_spec()
        assert spec is not None and spec[0] == target
        host = pg.transform(M_GRID)
        closed, _ = B.latent_transform(spec, M_GRID)
        err, nz = np.abs(closed - host), host != 0
        print(f"{target}/{act.name}: {(err[nz] / np.abs(host[nz])).max():.2e}")
        assert np.all(err <= 1e-13 * np.abs(host)), (target, act.name, (err[nz] / np.abs(host[nz])).max())


@pytest.mark.parametrize("target", ["lognormal", "normal", "uniform", "none"])
@pytest.mark.parametrize("act", ["identity", "softplus", "exp"])
def test_closed_form_derivatives_against_central_differences(B, target, act):
    """d(act ∘ target)/dm against central differences of its own value: eps = 1e-6, rtol 1e-5, atol 1e-8 — the rule of
    tests/test_oracle_crosscheck.py:142-149."""
    par = {"lognormal": (-0.7, 0.5), "normal": (1.0, 0.3), "uniform": (0.2, 2.0), "none": (0.0, 0.0)}[target]
    spec = (target, par, act, 0.1 if act == "softplus" else 0.0)
    eps = 1e-6
    _, dv = B.latent_transform(spec, M_GRID)
    fd = (B.latent_transform(spec, M_GRID + eps)[0] - B.latent_transform(spec, M_GRID - eps)[0]) / (2 * eps)
    assert np.allclose(dv, fd, rtol=1e-5, atol=1e-8), (target, act, np.abs(dv - fd).max())
