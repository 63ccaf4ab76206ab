"""Host-side checks of the posterior covariance of the gradient-observation and nonstationary models (no GPU needed):
the ABI is declared, exported and mirrored, NULL handles are refused without a device, and the new kernels keep the
register budget the hand-counted prefetch ring needs (csrc/gemm_f64.hpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("boss_ggp_predict_cov", "boss_ngp_predict_cov")


def test_cov_entry_points_declared_exported_and_mirrored():
    from boss_jl_amd import api
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "bosship.h")).read()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        assert hasattr(lib, s) and s in api.SIGNATURES
    assert len(api.SIGNATURES["boss_ggp_predict_cov"][1]) == 5 and len(api.SIGNATURES["boss_ngp_predict_cov"][1]) == 9
    assert hasattr(api.GradGP, "predict_value_cov") and "predict_cov" in vars(api.GibbsGP)


def test_cov_entry_points_refuse_a_null_handle():
    from boss_jl_amd import api
    lib = api.load_library()
    x, mu, cov = np.zeros(4), np.zeros(2), np.zeros(4)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    bad = C.c_long(0)
    assert lib.boss_ggp_predict_cov(None, 2, dp(x), dp(mu), dp(cov)) == api.BOSS_E_INVALID
    assert lib.boss_ngp_predict_cov(None, 2, dp(x), dp(x), dp(mu), None, dp(mu), dp(cov), C.byref(bad)) == api.BOSS_E_INVALID
    assert b"NULL" in lib.boss_last_error()


def test_cov_kernels_do_not_spill(tmp_path):
    out = tmp_path / "bosship.s"
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags +
                          ["-S", "--cuda-device-only", "-o", str(out), os.path.join(entry.CSRC, "bosship.hip")])
    txt = out.read_text()
    found = set()
    for m in re.finditer(r"\.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)", txt, re.S):
        agpr, name, scratch, vgpr = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
        for k in ("cov_syrk_partial_kernel", "cov_finish_kernel"):
            if k in name:
                found.add(name)
                assert agpr == 0 and scratch == 0 and vgpr <= 256, (name, agpr, scratch, vgpr)
    assert len(found) == 3, found                            # the partial kernel and both forms of the finish
