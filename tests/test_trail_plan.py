"""CPU-side replay of the deferred trailing-update plan under the resident chain (BOSS_CHAIN_TRAIL=4, trail_plan in
host_factor.inc, exported as boss_debug_trail_plan): for every chain size (3 … 64 block columns) and batch size, every
(strip, panel) pair is applied exactly once, in ascending panel order, before the panel solve or the chain reads the strip, and
the eight critical strips of step k are complete and counted before step k+1 reads them."""
import ctypes as C

import pytest

import __graft_entry__ as entry

BLK = 128


@pytest.fixture(scope="module")
def plan_fn():
    entry.build()
    from boss_jl_amd import api
    lib = api.load_library()
    fn = lib.boss_debug_trail_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]

    def plan(nblk, panels, lag):
        n = C.c_int(0)
        off = (C.c_int * nblk)()
        assert fn(nblk, panels, lag, C.byref(n), off, None, 0) == 0
        items = (C.c_int * (5 * max(n.value, 1)))()
        assert fn(nblk, panels, lag, C.byref(n), off, items, n.value) == 0
        rows = [tuple(items[5 * t:5 * t + 5]) for t in range(n.value)]
        return list(off), rows

    return plan


def replay(nblk, off, rows):
    """Walk the steps in launch order; returns the panels each strip received, in order."""
    applied = {}
    assert off[0] == 0 and off[nblk - 1] == len(rows)
    for k in range(nblk - 1):
        step = rows[off[k]:off[k + 1]]
        assert off[k] <= off[k + 1]
        seen = set()
        for R0, C0, k0, npan, crit in step:
            assert R0 % 32 == 0 and C0 % BLK == 0 and 1 <= npan <= 255
            r, j = R0 // 32, C0 // BLK
            assert (r, j) not in seen, "a strip is taken by two workgroups of one launch"
            seen.add((r, j))
            assert 1 <= j < nblk and 4 * j <= r <= 4 * nblk, (r, j)
            assert k0 + npan - 1 <= k, "a panel is applied before its solve"
            applied.setdefault((r, j), []).extend(range(k0, k0 + npan))
        ncrit = sum(c for *_, c in step)
        if k + 2 < nblk:
            # the eight critical strips, tiles (k+2, k+1) and (k+2, k+2), come first in the launch and are complete after it
            assert ncrit == 8 and all(c == 1 for *_, c in step[:8])
            crit = {(R0 // 32, C0 // BLK) for R0, C0, *_ in step[:8]}
            assert crit == {(4 * (k + 2) + s, j) for s in range(4) for j in (k + 1, k + 2)}
            for s in range(4):
                assert applied[(4 * (k + 2) + s, k + 1)] == list(range(k + 1))
                assert applied[(4 * (k + 2) + s, k + 2)] == list(range(k + 1))
        else:
            assert ncrit == 0
        # deadlines: block column k+1 (and its δ^T strip) is read by the panel solve of step k+1; tile (k+1, k+1) received its strips'
        # panels a step earlier (the chain kernel applies panel k itself)
        for r in list(range(4 * (k + 2), 4 * nblk)) + [4 * nblk]:
            assert applied.get((r, k + 1)) == list(range(k + 1)), (nblk, k, r, applied.get((r, k + 1)))
        for r in range(4 * (k + 1), 4 * (k + 2)):
            assert applied.get((r, k + 1), []) == list(range(k)), (nblk, k, r, applied.get((r, k + 1)))
    return applied


@pytest.mark.parametrize("panels,lag", [(1, 1), (2, 2), (3, 1), (4, 1), (4, 2), (4, 4), (8, 3)])
def test_deferred_plan_applies_every_panel_once_in_order(plan_fn, panels, lag):
    for nblk in range(3, 65):
        off, rows = plan_fn(nblk, panels, lag)
        applied = replay(nblk, off, rows)
        for (r, j), got in applied.items():                   # every panel exactly once, ascending (also beyond the deadlines above)
            want = list(range(j - 1)) if r // 4 == j else list(range(j))
            assert got == want, (nblk, r, j, got)
        for j in range(1, nblk):
            for r in range(4 * j, 4 * nblk + 1):
                assert (r, j) in applied or (r // 4 == j and j == 1), (nblk, r, j)


def test_deferred_plan_batches_far_work(plan_fn):
    """The point of the schedule, at its defaults for N = 4096 (32 block columns: P = 2 panels per batch, lag 1) and N = 8192 (64:
    P = 4, lag 3): most of the trailing work is applied in passes of P panels or more, the critical strips stay one panel deep,
    no step carries the pile of work mode 0's first steps do, and the strips of the late steps (few of them: the longest one is
    the launch) stay shallow."""
    for nblk, P, Q in ((32, 2, 1), (64, 4, 3)):
        off, rows = plan_fn(nblk, P, Q)
        panels = sum(r[3] for r in rows)
        assert panels == sum(4 * (j if i > j else j - 1) for j in range(1, nblk) for i in range(j, nblk)) + sum(range(1, nblk))
        assert sum(r[3] for r in rows if r[3] >= P) > 0.6 * panels
        for k in range(nblk - 2):
            assert all(r[3] == 1 for r in rows[off[k]:off[k] + 8]), k
        cost = [sum(r[3] + 0.7 for r in rows[off[k]:off[k + 1]]) for k in range(nblk - 1)]
        assert max(cost) < 2.5 * sum(cost) / len(cost)             # (mode 0 at k = 0: 2.9× the average at 32 block columns)
        assert max(r[3] for r in rows[off[nblk // 2]:off[nblk - 2]]) <= P + Q
