"""Host-side checks of the nonstationary append / reserve / tracked-candidates entry points (no GPU): the header, the Julia glue and
INTEGRATION.md name them, and the Python wrappers reject bad arguments before the library is touched."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("boss_ngp_reserve", "boss_ngp_track_create", "boss_ngp_track_create_lat")


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_entry_points_are_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", read("include", "bosship.h"), flags=re.S)
    jl = read("boss.jl_amd", "julia", "BOSSHip.jl")
    doc = read("INTEGRATION.md")
    from boss_jl_amd import api
    for sym in ABI:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert "(:%s, lib)" % sym in jl, sym
        assert "`%s`" % sym in doc and "(:%s, lib)" % sym in doc, sym
        assert sym in api.SIGNATURES, sym
    # the introspection call is exported by the library's source and bound by the Python twin; like every boss_debug_* it stays
    # out of the public header
    src = read("boss.jl_amd", "csrc", "host_append.inc")
    assert re.search(r'extern "C" int boss_debug_append_path\(const boss_gp_t\* \w+, int\* path_out\)', src)
    assert "boss_debug_append_path" not in header and "boss_debug_append_path" in read("boss.jl_amd", "api.py")
    assert callable(api._append_path) and callable(api.GibbsGP.reserve) and api.GibbsGP.reserve is not api.GP.reserve
    # the header says what the append now does, and nobody claims a rebuild any more
    full = read("include", "bosship.h")
    blk = full[full.index("augment_dataset! (src/types/problem.jl:191-198) for a fitted nonstationary posterior"):]
    blk = blk[:blk.index("int boss_ngp_append(")]
    assert "equals a fresh fit of the augmented data" in blk and "to rounding" in blk and "rebuilt and factorised" not in blk
    for path in (("boss.jl_amd", "api.py"), ("boss.jl_amd", "nonstationary.py")):
        assert "rebuilt and factorised (boss_ngp_append)" not in read(*path), path
    assert "couples every pair of points" not in read("boss.jl_amd", "csrc", "host_factor.inc") + src


class FakeCand:
    d, M, _h = 3, 5, None


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched: " + name)


def test_gibbs_track_checks_its_arguments_first(monkeypatch):
    from boss_jl_amd import api
    monkeypatch.setattr(api, "load_library", lambda path=None: Untouchable())
    cand, gp = FakeCand(), object()
    lam, amp = np.ones((3, 5)), np.ones(5)
    lat = object.__new__(api.NgpLatents)
    lat._h = 1
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand)                                # neither
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand, lam, amp, latents=lat)         # both
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand, lam_Xs=lam)                    # half of the arrays
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand, amp_Xs=amp, latents=lat)
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand, np.ones((5, 3)), amp)          # wrong shapes
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand, lam, np.ones(4))
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand, lam, amp, mean_Xs=np.ones(6))
    with pytest.raises(ValueError):
        api.GibbsTrack(gp, cand, latents="not a latent object")
    lat._h = None                                               # (keeps __del__ away from the fake library)
    assert issubclass(api.GibbsTrack, api.Track)


def test_sequential_batch_checks_its_arguments_first(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api, nonstationary
    monkeypatch.setattr(api, "load_library", lambda path=None: Untouchable())
    Xs = np.zeros((3, 4))
    with pytest.raises(ValueError):
        nonstationary.nonstationary_sequential_batch([[object()]], Xs, 0, [1.0])
    with pytest.raises(ValueError):
        nonstationary.nonstationary_sequential_batch([], Xs, 2, [1.0])
    with pytest.raises(ValueError):
        nonstationary.nonstationary_sequential_batch([[]], Xs, 2, [1.0])
    assert B.nonstationary_sequential_batch is nonstationary.nonstationary_sequential_batch
    assert callable(nonstationary.HipNonstationaryPosteriorSlice.track)
