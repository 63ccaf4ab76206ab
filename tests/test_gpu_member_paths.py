"""Which entry point may take the set launches (pytest -m gpu): the `allow_set` argument every caller of members_enqueue
(csrc/host_predict.inc) passes, row by row, read off the launch counters api._set_launches() / api._set_grad_launches().

    entry point                                                  set launches
    boss_acq_ei_grad, boss_acq_ei_grad_set with S = 1            never
    boss_acq_ei_grad_set with S > 1                              always
    boss_acq_ei_mc_grad                                          any S, S = 1 included (its P >= 2 members qualify)
    boss_ngp_predict_set, _grad_set, boss_ngp_acq_ei_grad_set    always, any S
    boss_warp_predict, boss_warp_predict_grad                    never
    boss_acq_ei_warp, boss_acq_ei_grad_warp                      S > 1 only
    boss_acq_ei / boss_acq_ei_mc on handles                      S > 1 and a mode other than 0

"Always" means: where the members allow it — a list of unequal N and a program-kernel handle go member by member everywhere.
Rows other tests hold already are cited, not repeated:
  boss_acq_ei_grad_set, S > 1 (plain and gradient-observation members)     tests/test_gpu_acq_grad_set.py::test_path_and_determinism
  boss_acq_ei_grad_set, unequal N                                         tests/test_gpu_acq_grad_set.py::test_mixed_shapes_go_member_by_member
  boss_ngp_predict_set                                                    tests/test_gpu_model_fit_batch.py (the _set_launches()[1] assertion)
  boss_ngp_predict_grad_set / boss_ngp_acq_ei_grad_set, S > 1             tests/test_gpu_ngp_grad_set.py (run_case's counter assertions)
  the _lat forms                                                          tests/test_gpu_nlat.py (the _set_grad_launches assertions)
  boss_acq_ei on handles, S > 1                                           tests/test_gpu_fit_batch.py, tests/test_gpu_model_fit_batch.py
Shapes: d = 3, N = 130, M = 33 (one full and one partial tile of 32), P = 2, S = 3: the smallest at which the set paths exist
(N > 128: below, the one-launch small kernel replaces the set gradient path).
"""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SET = os.environ.get("BOSS_NO_SET_PREDICT") == "1"
D, N, M, P, S = 3, 130, 33, 2, 3


@pytest.fixture(scope="module")
def api():
    entry.build()
    from boss_jl_amd import api as a
    a.load_library()
    assert a.device_count() >= 1
    return a


@pytest.fixture(scope="module")
def T():
    """the builders of tools/members_fold_dump.py (members, fitness, warp and kernel programs)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import members_fold_dump
    return members_fold_dump


@pytest.fixture(scope="module")
def case(api, T):
    rng = np.random.default_rng(5)
    gps, mean, gr, Y = T.plain_members(api, rng, N, S=S)
    Xs = np.asfortranarray(rng.uniform(0.02, 0.98, (D, M)))
    ms, mg = T.means_at(mean, gr, P, S, Xs)
    c = dict(gps=gps, Xs=Xs, ms=ms, mg=mg, cand=api.Candidates(Xs), best=float(Y[0].max()) - 0.3, coefs=[1.0, 0.2], ymax=[np.inf, 0.3],
             fit=T.fitness(api, P), eps1=rng.standard_normal((P, 8)), epsS=rng.standard_normal((P, S)), warps=T.warps(api, P))
    yield c
    c["cand"].close(), c["fit"].close()
    for w in c["warps"].values():
        w.close()
    for row in gps:
        for g in row:
            g.close()


def deltas(api, fn):
    """(rise of the set-prediction launches, rise of the set adjoint launches) over fn()"""
    before = (api._set_launches()[0], api._set_grad_launches())
    fn()
    return api._set_launches()[0] - before[0], api._set_grad_launches() - before[1]


def member_by_member(api, fn, what):
    assert deltas(api, fn) == (0, 0), f"{what} took the set launches"


def set_path(api, fn, what, grad):
    dp, dg = deltas(api, fn)
    print(f"{what}: set-prediction launches +{dp}, set adjoint launches +{dg}", flush=True)
    if NO_SET:
        assert (dp, dg) == (0, 0), f"{what} took the set launches under BOSS_NO_SET_PREDICT=1"
    else:
        assert dp > 0 and (dg > 0) == grad, f"{what}: (+{dp}, +{dg}), expected the set {'gradient' if grad else 'prediction'} path"


def test_one_sample_gradient_calls_never_take_the_set_launches(api, case):
    c = case
    one = c["gps"][0]                                            # P = 2 members of one shape: the predicate alone would let them through
    member_by_member(api, lambda: api.acq_ei_grad(one, c["Xs"], c["coefs"], c["ymax"], c["best"], None, c["ms"][0], c["mg"][0]), "acq_ei_grad")
    member_by_member(api, lambda: api.acq_ei_grad_set([one], c["Xs"], c["coefs"], c["ymax"], c["best"], None, c["ms"][:1], c["mg"][:1]),
                     "acq_ei_grad_set, S = 1")


def test_monte_carlo_gradient_takes_them_at_any_S(api, case):
    c = case
    set_path(api, lambda: api.acq_ei_mc_grad(c["gps"][:1], c["Xs"], c["fit"], c["eps1"], c["ymax"], c["best"], None, c["ms"][:1], c["mg"][:1]),
             "acq_ei_mc_grad, S = 1, P = 2", grad=True)
    set_path(api, lambda: api.acq_ei_mc_grad(c["gps"], c["Xs"], c["fit"], c["epsS"], c["ymax"], c["best"], None, c["ms"], c["mg"]),
             "acq_ei_mc_grad, S = 3", grad=True)


def test_value_calls_on_handles_take_them_for_S_above_one_in_a_predicting_mode(api, case):
    c = case
    set_path(api, lambda: api.acq_ei(c["gps"], c["cand"], c["coefs"], c["ymax"], c["best"], None, c["ms"]), "acq_ei, S = 3", grad=False)
    set_path(api, lambda: api.acq_ei_mc(c["gps"], c["cand"], c["fit"], c["epsS"], c["ymax"], c["best"], None, c["ms"]), "acq_ei_mc, S = 3", grad=False)
    member_by_member(api, lambda: api.acq_ei(c["gps"][:1], c["cand"], c["coefs"], c["ymax"], c["best"], None, c["ms"][:1]), "acq_ei, S = 1")
    member_by_member(api, lambda: api.acq_ei_mc(c["gps"][:1], c["cand"], c["fit"], c["eps1"], c["ymax"], c["best"], None, c["ms"][:1]), "acq_ei_mc, S = 1")
    member_by_member(api, lambda: api.acq_ei(c["gps"], c["cand"], c["coefs"]), "acq_ei, S = 3, mode 0 (nothing is predicted)")


@pytest.mark.parametrize("which", ["in", "out", "both"])
def test_warp_calls(api, case, which):
    c = case
    w = c["warps"][which]
    member_by_member(api, lambda: w.predict(c["gps"], c["Xs"], c["ms"]), f"warp {which}: predict, S = 3")
    member_by_member(api, lambda: w.predict_grad(c["gps"], c["Xs"], c["ms"], c["mg"]), f"warp {which}: predict_grad, S = 3")
    member_by_member(api, lambda: w.acq_ei(c["gps"][:1], c["Xs"], c["coefs"], c["ymax"], c["best"], None, c["ms"][:1]), f"warp {which}: acq_ei, S = 1")
    member_by_member(api, lambda: w.acq_ei_grad(c["gps"][:1], c["Xs"], c["coefs"], c["ymax"], c["best"], None, c["ms"][:1], c["mg"][:1]),
                     f"warp {which}: acq_ei_grad, S = 1")
    set_path(api, lambda: w.acq_ei(c["gps"], c["Xs"], c["coefs"], c["ymax"], c["best"], None, c["ms"]), f"warp {which}: acq_ei, S = 3", grad=False)
    set_path(api, lambda: w.acq_ei_grad(c["gps"], c["Xs"], c["coefs"], c["ymax"], c["best"], None, c["ms"], c["mg"]),
             f"warp {which}: acq_ei_grad, S = 3", grad=True)


def test_nonstationary_acquisition_takes_them_at_S_one(api):
    """boss_ngp_acq_ei_grad_set with S = 1: its P = 2 members (two outputs fitted on one X) take the set launches"""
    rng = np.random.default_rng(6)
    X = rng.uniform(0, 1, (D, N))
    Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1]])
    lam, amp = (0.5 + 0.2 * X)[:, :, None], (1.0 + 0.3 * X[0])[:, None]
    gps = [api.ngp_fit_batch(X, Y[p], lam, amp, np.full((N, 1), 0.07))[0][0] for p in range(P)]
    Xs = np.asfortranarray(rng.uniform(0.02, 0.98, (D, M)))
    lam_s, amp_s = np.repeat((0.5 + 0.2 * Xs)[:, :, None], P, axis=2), np.repeat((1.0 + 0.3 * Xs[0])[:, None], P, axis=1)
    try:
        set_path(api, lambda: api.ngp_acq_ei_grad_set([gps], Xs, lam_s, amp_s, None, None, [1.0, 0.2], None, 0.4), "ngp_acq_ei_grad_set, S = 1", grad=True)
    finally:
        for g in gps:
            g.close()


def test_unequal_members_and_program_kernels_go_member_by_member(api, case, T):
    c = case
    rng = np.random.default_rng(7)
    other, _, _, _ = T.plain_members(api, rng, N + 10, S=1)
    rows = [[c["gps"][0][0]], [other[0][0]], [c["gps"][1][0]]]
    fit1, w1 = T.fitness(api, 1), T.warps(api, 1)["both"]
    eps = rng.standard_normal((1, 3))
    X = rng.uniform(0, 1, (D, N))
    prog = T.sqexp_program(api)
    ks = [api.KernelGP(X, np.sin(3 * X).sum(0), prog, grad=True) for _ in range(S)]
    try:
        member_by_member(api, lambda: api.acq_ei(rows, c["cand"], [1.0], None, c["best"]), "acq_ei, unequal N")
        member_by_member(api, lambda: api.acq_ei_mc_grad(rows, c["Xs"], fit1, eps, None, c["best"]), "acq_ei_mc_grad, unequal N")
        member_by_member(api, lambda: w1.acq_ei(rows, c["Xs"], [1.0], None, c["best"]), "warp acq_ei, unequal N")
        member_by_member(api, lambda: w1.acq_ei_grad(rows, c["Xs"], [1.0], None, c["best"]), "warp acq_ei_grad, unequal N")
        for s, g in enumerate(ks):
            g.update([0.5 + 0.05 * s, 0.6, 0.7], 1.0, 0.05)
        krows = [[g] for g in ks]
        member_by_member(api, lambda: api.acq_ei(krows, c["cand"], [1.0], None, c["best"]), "acq_ei, program kernel")
        member_by_member(api, lambda: api.acq_ei_grad_set(krows, c["Xs"], [1.0], None, c["best"]), "acq_ei_grad_set, program kernel")
    finally:
        for g in ks + [other[0][0], other[0][1]]:
            g.close()
        prog.close(), fit1.close(), w1.close()
