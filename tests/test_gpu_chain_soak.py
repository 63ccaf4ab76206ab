"""Soak tests of the resident panel chain (csrc/chain.hpp), pytest -m gpu.

The chain is a lock-free protocol between workgroups that run at the same time (write-through stores, sequence words, data-pattern
polling).  Its arithmetic order is fixed — whichever of its paths a wave takes (one or two panels per round trip, lockstep or late
strips) issues the same MFMAs on the same operands in the same order — so repeated updates under the same hyper-parameters must be
BIT-IDENTICAL: logpdf and the whole factor.  A hand-off that lets a consumer read a tile too early, or apply a panel twice, shows
up as a changed bit long before it exceeds a parity tolerance.  (Replaces the schedule around AbstractGPs.posterior's cholesky,
/root/reference/src/models/gaussian_process.jl:199-211.)
"""
import struct
import threading

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

LEVELS = [0.05 + 1e-4 * i for i in range(7)]


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


def make(d, N, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(2 * np.pi * X).sum(0) / np.sqrt(d) + 0.05 * rng.standard_normal(N)
    return X, y


def bits(x):
    return struct.pack("<d", float(x))


def soak(api, N, updates, with_load):
    d = 8
    X, y = make(d, N, 11)
    lam = np.full(d, 0.5)
    g = api.GP(X, y, "matern52")
    stop = threading.Event()
    load_calls = [0]
    load_err = []
    th = None
    if with_load:
        # a second host thread keeps the device busy with 8192-candidate acquisitions on ANOTHER handle of the same device
        # context: its kernels share the main stream, the CUs and the L2 with the chain
        X2, y2 = make(d, 2048, 12)
        g2 = api.GP(X2, y2, "matern52")
        g2.update(lam, 1.0, 0.05)
        cand = api.Candidates(np.random.default_rng(13).uniform(0, 1, (d, 8192)))
        best = float(y2.max())
        ref = api.acq_ei([[g2]], cand, [1.0], None, best, want_acq=False)[1:]

        def load():
            try:
                while not stop.is_set():
                    got = api.acq_ei([[g2]], cand, [1.0], None, best, want_acq=False)[1:]
                    if got != ref:
                        load_err.append((got, ref))
                        return
                    load_calls[0] += 1
            except Exception as e:                               # surfaces in the main thread's assertion
                load_err.append(repr(e))

        th = threading.Thread(target=load, daemon=True)
        th.start()
    first_lp, first_L = {}, {}
    changed = []
    try:
        for i in range(updates):
            lv = i % len(LEVELS)
            lp = g.update(lam, 1.0, LEVELS[lv])
            if lv not in first_lp:
                first_lp[lv] = lp
                first_L[lv] = g.factor()
            elif bits(lp) != bits(first_lp[lv]):
                changed.append((i, lv, lp, first_lp[lv]))
            # the whole factor of every level once more near the end of the run
            if i >= updates - len(LEVELS):
                L, z = g.factor()
                if not (np.array_equal(L, first_L[lv][0]) and np.array_equal(z, first_L[lv][1])):
                    changed.append((i, lv, "factor"))
    finally:
        stop.set()
        if th is not None:
            th.join(timeout=60)
    assert not load_err, load_err[:2]
    assert not changed, f"{len(changed)} of {updates} updates differ from the first occurrence of their level: {changed[:4]}"
    if with_load:
        assert load_calls[0] >= 3, load_calls                      # the load really ran beside the updates
    g.close()
    return load_calls[0]


@pytest.mark.parametrize("N", [1408, 4096])
def test_repeated_updates_are_bit_identical(api, N):
    """500 updates cycling 7 noise levels: every repeat of a level equals its first occurrence bit for bit."""
    soak(api, N, 500, with_load=False)


@pytest.mark.parametrize("N", [1408, 4096])
def test_repeated_updates_are_bit_identical_under_load(api, N):
    """The same while a second host thread runs 8192-candidate acquisitions on another handle of the device."""
    soak(api, N, 500, with_load=True)


def foreign_load_soak(api, N, updates):
    """Updates beside work the library knows nothing about: a torch thread on a HIP stream of its own, in the same process, running
    fp64 matrix products (rocBLAS, every CU) and large device copies.  Nothing of it takes the library's mutex or streams — its
    kernels really are on the device while the chain's resident workgroups poll."""
    import ctypes as C
    import torch
    lib = api.load_library()
    d = 8
    X, y = make(d, N, 21)
    lam = np.full(d, 0.5)
    g = api.GP(X, y, "matern52")
    ref = {}
    for lv, s in enumerate(LEVELS):                              # the undisturbed results first
        lp = g.update(lam, 1.0, s)
        ref[lv] = (lp, g.factor())
    fb0, off0 = C.c_long(0), C.c_int(0)
    lib.boss_debug_fallbacks(0, C.byref(fb0), C.byref(off0))
    stop = threading.Event()
    done = [0]
    err = []

    def load():
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                a = torch.randn(4096, 4096, dtype=torch.float64, device="cuda")
                b = torch.randn(4096, 4096, dtype=torch.float64, device="cuda")
                big = torch.empty(64 * 1024 * 1024, dtype=torch.float64, device="cuda")     # 512 MB
                dst = torch.empty_like(big)
                while not stop.is_set():
                    c = a @ b
                    dst.copy_(big, non_blocking=True)
                    a = c / c.abs().max()
                    st.synchronize()
                    done[0] += 1
        except Exception as e:
            err.append(repr(e))

    th = threading.Thread(target=load, daemon=True)
    th.start()
    changed = []
    try:
        while done[0] < 2 and not err:                           # the foreign work is on the device before the first update
            pass
        for i in range(updates):
            lv = i % len(LEVELS)
            lp = g.update(lam, 1.0, LEVELS[lv])
            if bits(lp) != bits(ref[lv][0]):
                changed.append((i, lv, lp, ref[lv][0]))
            if i >= updates - len(LEVELS):
                L, z = g.factor()
                if not (np.array_equal(L, ref[lv][1][0]) and np.array_equal(z, ref[lv][1][1])):
                    changed.append((i, lv, "factor"))
    finally:
        stop.set()
        th.join(timeout=120)
    fb1, off1 = C.c_long(0), C.c_int(0)
    lib.boss_debug_fallbacks(0, C.byref(fb1), C.byref(off1))
    g.close()
    return changed, err, done[0], fb1.value - fb0.value, off1.value


@pytest.mark.parametrize("N", [1408, 4096])
def test_updates_beside_foreign_kernels_are_bit_identical(api, N):
    """500 updates while a torch stream of the same process keeps every CU busy with fp64 GEMMs and 512 MB copies: logpdf and factor
    equal the undisturbed results bit for bit.  Whether the resident chain keeps up beside kernels that hold every CU for milliseconds
    is the device's business: an update whose waits ran out of their budget is repeated on the simpler schedule (announced once on
    stderr, counted here) — the numbers must not depend on who else uses the GPU (gaussian_process.jl:199-211 has no such notion)."""
    changed, err, loops, fallbacks, chain_off = foreign_load_soak(api, N, 500)
    assert not err, err
    assert loops >= 5, loops                                      # the foreign work really ran beside the updates
    assert not changed, f"{len(changed)} of 500 updates differ from the undisturbed result: {changed[:4]} (fallbacks {fallbacks})"
    assert fallbacks <= 2, fallbacks                              # at most: chain off once, then at most one gate fallback (each is taken once per process / context)
    print(f"N={N}: foreign loops {loops}, fallbacks {fallbacks}, chain switched off {chain_off}")


def test_cu_masked_streams_are_bit_identical(tmp_path):
    """The round-3 experiment that once gave wrong factors: chain and strips on reserved CUs, the update's other kernels on the
    complement (hipExtStreamCreateWithCUMask, BOSS_CU_MASK=1), i.e. every hand-off of the protocol crosses hardware queues AND CU
    sets.  A run with masked streams must reproduce the unmasked run bit for bit — logpdf of every update, the factor of the first and
    last ones, the fused update + acquisition — without a fallback (tools/cumask_check.py exits non-zero on any difference).  The
    masks are fixed when a context is created, hence the two child processes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NS="1408,4096", NHASH="2", LONG="90", CUMASK_DIR=str(tmp_path))
    env.pop("BOSS_CU_MASK", None)
    tool = os.path.join(root, "tools", "cumask_check.py")
    rec = subprocess.run([sys.executable, tool, "record", "12"], env=env, capture_output=True, text=True, timeout=300)
    assert rec.returncode == 0, rec.stdout[-2000:] + rec.stderr[-2000:]
    chk = subprocess.run([sys.executable, tool, "check", "12"], env=dict(env, BOSS_CU_MASK="1"), capture_output=True, text=True, timeout=300)
    assert chk.returncode == 0, chk.stdout[-2000:] + chk.stderr[-2000:]
    assert "MISMATCHES: 0" in chk.stdout and "BOSS_CU_MASK=1" in chk.stderr, chk.stdout[-2000:] + chk.stderr[-500:]
    assert "fallbacks so far 0" in chk.stdout, chk.stdout[-2000:]
