"""Program-kernel posteriors in batches (boss_kgp_loglike_batch, boss_kgp_fit_batch) and as a set in one prediction launch
(predict_set_enqueue over kprog_kstar_set_kernel), up to the Python surface of a HipGaussianProcess under a DeviceKernel.

References.  (a) The single-handle path: boss_kgp_create + boss_gp_update at the same parameters — compared with `==` wherever the
batched route evaluates the same entries in the same order (Gram entries, likelihoods, factors, member predictions, and the set
route's moments: kprog_kstar_set_kernel and predict_kernel_set<G, true> run the bodies of kprog_kstar_kernel<32> and
predict_kernel<G32, true>).  (b) The restatement of tests/test_gpu_kernel_program.py (kernel_program_cases.Restated: K from the
closure, scipy Cholesky) at its tolerance tol = max(1e-9, cond(K)·N·2⁻⁵³·8), applied as there.

Cases, the smallest at which each piece can go wrong (N: partial 64-tiles; 128-padded batches of 128 / 256 / 384 rows beside
256-padded handles of 256 / 256 / 512 rows; more than one 256-row step):
  e1    exponential kernel, d = 1,  N = 70    5 instructions: four waves per workgroup
  dot3  u·v + 1,            d = 3,  N = 130   the prior variance differs per candidate
  f16   64 instructions,    d = 16, N = 300   96 LDS slots per thread: one wave per workgroup
  e3d   exponential kernel, d = 3,  N = 130   one discrete dimension, a prior mean

The moments of the set route are not returned by any entry point of their own; they are seen through boss_acq_ei, whose values over a
set are compared bit for bit with the epilogue on the member-by-member moments (boss_acq_ei_moments on boss_gp_predict's output)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                      # (run as a script, the module is the child of the chunk test)
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
import kernel_program_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

AMP = 1.0
S_ALL = 9                                                     # the parameter sets of a case; S = 2 and 8 are its prefixes


def full16(u, v):
    """Matérn-5/2 × inverse multiquadric × squared exponential + squared exponential: 64 instructions at d = 16."""
    r2 = cases._r2(u, v)
    s = np.sqrt(5.0 * r2)
    q = (1 + s + 5.0 / 3.0 * r2) * np.exp(-s)
    return q * (1 / (1 + r2)) * np.exp(-0.125 * r2) + np.exp(-0.5 * r2)


CLOSURES = dict(cases.CLOSURES, full16=full16)
CASES = {
    "e1": dict(name="expo", d=1, N=70, noise=0.05),
    "dot3": dict(name="dot1", d=3, N=130, noise=0.1),
    "f16": dict(name="full16", d=16, N=300, noise=0.05),
    "e3d": dict(name="expo", d=3, N=130, noise=0.05, discrete=[False, True, False], scale=[1.0, 4.0, 1.0], mean=True),
}
M_MAX = 70


@pytest.fixture(scope="module")
def B():
    entry.build()
    import boss_jl_amd as B
    B.api.load_library()
    assert B.api.device_count() >= 1
    return B


@pytest.fixture(scope="module")
def api(B):
    return B.api


_kernels, _setups, _singles, _restated = {}, {}, {}, {}


def kernel_of(B, name, d):
    if (name, d) not in _kernels:
        _kernels[(name, d)] = B.DeviceKernel(CLOSURES[name], d)
    return _kernels[(name, d)]


def setup(case):
    """(X, y, Xs, lam d×9, amp, sig, discrete, mean_X, mean_Xs) of a case, computed once and shared."""
    if case not in _setups:
        c = CASES[case]
        d, sc = c["d"], np.asarray(c.get("scale", np.ones(c["d"])), float)
        X, y, Xs = cases.data(d, c["N"], M_MAX, seed=21, scale=sc)
        k = np.arange(S_ALL)
        lam = (np.linspace(0.4, 0.6, d) * sc)[:, None] * (1.0 + 0.1 * k)[None, :]
        amp, sig = AMP + 0.05 * k, c["noise"] * (1.0 + 0.1 * k)
        mX = 0.5 + 0.2 * X.sum(0) if c.get("mean") else None
        mXs = 0.5 + 0.2 * Xs.sum(0) if c.get("mean") else None
        for a in (X, y, Xs, lam, amp, sig):
            a.setflags(write=False)
        _setups[case] = (X, y, Xs, lam, amp, sig, c.get("discrete"), mX, mXs)
    return _setups[case]


def program(B, case):
    return kernel_of(B, CASES[case]["name"], CASES[case]["d"]).program


def single(B, case, s, y=None):
    """A create + update handle at parameter set s (the caller closes it)."""
    X, y0, _, lam, amp, sig, disc, mX, _ = setup(case)
    g = B.api.KernelGP(X, y0 if y is None else y, program(B, case), disc)
    g.update(lam[:, s], amp[s], sig[s], mX)
    return g


def single_logpdfs(B, case):
    """logpdf of S_ALL updates on ONE handle: the loop the batched call replaces."""
    if case not in _singles:
        X, y, _, lam, amp, sig, disc, mX, _ = setup(case)
        g = B.api.KernelGP(X, y, program(B, case), disc)
        try:
            _singles[case] = np.array([g.update(lam[:, s], amp[s], sig[s], mX) for s in range(S_ALL)])
        finally:
            g.close()
    return _singles[case]


def restated(case, s, with_pred=False):
    key = (case, s)
    if key not in _restated:
        X, y, Xs, lam, amp, sig, disc, mX, mXs = setup(case)
        _restated[key] = cases.Restated(CLOSURES[CASES[case]["name"]], X, y, lam[:, s], amp[s], sig[s], Xs, disc, mX, mXs)
    return _restated[key]


def close_all(gps):
    for g in gps:
        g.close()


def test_the_programs_cover_both_ends_of_the_workgroup_sizing(B):
    """kprog_block: as many of 4 waves as fit 64 KiB at 8·64·(2d + n_instr) bytes per wave."""
    waves = lambda p: max(1, min(4, 65536 // (8 * 64 * (2 * p.d + p.code.shape[0]))))
    short, full = program(B, "e1"), program(B, "f16")
    assert short.code.shape[0] == 5 and waves(short) == 4
    assert full.code.shape[0] == B.api.FIT_MAX_INSTR == 64 and full.d == 16 and waves(full) == 1
    assert waves(program(B, "dot3")) == 4


# ------------------------------------------------------------------------------------------ likelihoods
@pytest.mark.parametrize("S", [2, 8, 9])
@pytest.mark.parametrize("case", sorted(CASES))
def test_batched_likelihoods_equal_single_updates(B, api, case, S):
    """S = 2 and 8 take the look-ahead schedule of the batched factorisation, 9 its paired panels."""
    X, y, _, lam, amp, sig, disc, mX, _ = setup(case)
    ll, st = api.kgp_loglike_batch(X, y, program(B, case), lam[:, :S], amp[:S], sig[:S], mX, disc)
    want = single_logpdfs(B, case)[:S]
    print(f"[kprog batch] {case} S={S}: max|ll - single| {np.abs(ll - want).max():.3e}")
    assert not st.any()
    assert np.array_equal(ll, want)
    ll2, _ = api.kgp_loglike_batch(X, y, program(B, case), lam[:, :S], amp[:S], sig[:S], mX, disc)
    assert np.array_equal(ll, ll2)                            # no atomics: repeated calls agree bit for bit
    if mX is not None:                                        # one prior-mean row per set
        ll3, _ = api.kgp_loglike_batch(X, y, program(B, case), lam[:, :S], amp[:S], sig[:S], np.tile(mX, (S, 1)), disc)
        assert np.array_equal(ll, ll3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_batched_likelihoods_match_the_restatement(B, api, case):
    X, y, _, lam, amp, sig, disc, mX, _ = setup(case)
    ll, st = api.kgp_loglike_batch(X, y, program(B, case), lam, amp, sig, mX, disc)
    assert not st.any()
    for s in (0, 4, 8):
        ref = restated(case, s)
        print(f"[kprog batch] {case} set {s}: cond {ref.cond:.3e} tol {ref.tol:.3e} |dlogpdf| {abs(ll[s] - ref.logpdf):.3e} "
              f"(bound {ref.tol * (1 + abs(ref.logpdf)):.3e})")
        assert ref.cond < 1e6
        assert abs(ll[s] - ref.logpdf) <= ref.tol * (1 + abs(ref.logpdf))


def chunk_call(api, B):
    X, y, _, lam, amp, sig, disc, mX, _ = setup("dot3")
    return api.kgp_loglike_batch(X, y, program(B, "dot3"), lam, amp, sig, mX, disc)


def test_chunks_agree_bitwise_with_one_batch(B, api, tmp_path):
    """BOSS_MODEL_BATCH_CHUNK_MB=2 (read once per process, so in a child) cuts the 9 matrices of 576 KiB (256 + 32 rows × 256
    columns) into three chunks of 3."""
    out = os.path.join(str(tmp_path), "child.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, BOSS_MODEL_BATCH_CHUNK_MB="2"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    child = np.load(out)
    ll, st = chunk_call(api, B)
    assert not st.any() and np.isfinite(ll).all()
    assert np.array_equal(child["ll"], ll) and np.array_equal(child["st"], st)
    assert np.array_equal(ll, single_logpdfs(B, "dot3"))


def test_failures_stay_local(B, api):
    """An invalid set (negative amplitude) and a set that is not positive definite (u·v + 1 has rank d + 1, σ = 0) get -inf and
    their status; their neighbours are those of the clean batch."""
    X, y, _, lam, amp, sig, disc, mX, _ = setup("dot3")
    S = 5
    a2, s2 = amp[:S].copy(), sig[:S].copy()
    a2[1], s2[3] = -1.0, 0.0
    ll, st = api.kgp_loglike_batch(X, y, program(B, "dot3"), lam[:, :S], a2, s2)
    clean = single_logpdfs(B, "dot3")
    assert list(st) == [0, api.BOSS_E_INVALID, 0, api.BOSS_E_NOT_PD, 0]
    assert ll[1] == -np.inf and ll[3] == -np.inf
    assert np.array_equal(ll[[0, 2, 4]], clean[[0, 2, 4]])
    g = api.KernelGP(X, y, program(B, "dot3"))                # the single handle says the same of set 3
    try:
        with pytest.raises(api.PosDefException):
            g.update(lam[:, 3], amp[3], 0.0)
    finally:
        g.close()
    gps, lp, st2 = api.kgp_fit_batch(X, y, program(B, "dot3"), lam[:, :S], np.abs(a2), s2)
    try:
        assert list(st2) == [0, 0, 0, api.BOSS_E_NOT_PD, 0] and lp[3] == -np.inf and gps[3].logpdf is None
        with pytest.raises(api.BossError) as e:
            gps[3].predict(X[:, :2])
        assert e.value.code == api.BOSS_E_NOT_FITTED
        assert np.array_equal(lp[[0, 2, 4]], clean[[0, 2, 4]])
    finally:
        close_all(gps)


# ------------------------------------------------------------------------------------------ fitted sets
@pytest.mark.parametrize("case", sorted(CASES))
def test_members_equal_create_and_update_handles(B, api, case):
    X, y, Xs, lam, amp, sig, disc, mX, mXs = setup(case)
    S = 3
    gps, lp, st = api.kgp_fit_batch(X, y, program(B, case), lam[:, :S], amp[:S], sig[:S], mX, disc)
    ones = []
    try:
        assert not st.any() and np.array_equal(lp, single_logpdfs(B, case)[:S])
        for s in range(S):
            ones.append(single(B, case, s))
            assert gps[s].logpdf == ones[s].logpdf
            (L, z), (L1, z1) = gps[s].factor(), ones[s].factor()
            assert np.array_equal(L, L1) and np.array_equal(z, z1), s
            for M in (1, M_MAX):
                (mu, var), (mu1, var1) = gps[s].predict(Xs[:, :M], None if mXs is None else mXs[:M]), \
                    ones[s].predict(Xs[:, :M], None if mXs is None else mXs[:M])
                assert np.array_equal(mu, mu1) and np.array_equal(var, var1), (s, M)
        ref = restated(case, 0)
        mu, var = gps[0].predict(Xs, mXs)
        assert np.abs(mu - ref.mu).max() <= ref.tol * (1 + np.abs(ref.mu).max())
        assert np.abs(var - np.where((ref.var < 0) & (ref.var >= -1e-8), 0.0, ref.var)).max() <= ref.tol * ref.kss.max()
        # a member is a program handle for every call that refuses one
        for call in (lambda: gps[0].append(Xs[:, 0], 0.0), lambda: gps[0].predict_cov(Xs[:, :3])):
            with pytest.raises(api.BossError) as e:
                call()
            assert e.value.code == api.BOSS_E_INVALID and "program-kernel posteriors" in str(e.value)
        # updating a member (here at the parameters of set 5) leaves its siblings as they were; new observations detach it
        before = [gps[s].predict(Xs, mXs) for s in (0, 2)]
        lp5 = gps[1].update(lam[:, 5], amp[5], sig[5], mX)
        assert lp5 == single_logpdfs(B, case)[5]
        y2 = y[::-1].copy()
        gps[1].set_y(y2)
        lp5b = gps[1].update(lam[:, 5], amp[5], sig[5], mX)
        one5 = single(B, case, 5, y2)
        ones.append(one5)
        assert lp5b == one5.logpdf
        (mu, var), (mu1, var1) = gps[1].predict(Xs, mXs), one5.predict(Xs, mXs)
        assert np.array_equal(mu, mu1) and np.array_equal(var, var1)
        after = [gps[s].predict(Xs, mXs) for s in (0, 2)]
        for (m0, v0), (m1, v1) in zip(before, after):
            assert np.array_equal(m0, m1) and np.array_equal(v0, v1)
        assert gps[0].update(lam[:, 0], amp[0], sig[0], mX) == lp[0]
    finally:
        close_all(gps + ones)


def test_gradients_on_a_member(B, api):
    """boss_kgp_set_grad on a member, then boss_gp_predict_grad and boss_gp_loglike_grad: the single flagged handle's values."""
    X, y, Xs, lam, amp, sig, disc, mX, mXs = setup("dot3")
    gps, _, st = api.kgp_fit_batch(X, y, program(B, "dot3"), lam[:, :2], amp[:2], sig[:2], grad=True)
    one = api.KernelGP(X, y, program(B, "dot3"), grad=True)
    try:
        assert not st.any() and all(g.grad for g in gps)
        one.update(lam[:, 1], amp[1], sig[1])
        got, want = gps[1].predict_grad(Xs[:, :33]), one.predict_grad(Xs[:, :33])
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        (l0, g0), (l1, g1) = gps[1].loglike_grad(), one.loglike_grad()
        assert l0 == l1 and np.array_equal(g0, g1)
        api._check(api.load_library().boss_kgp_set_grad(gps[0]._h, 0))   # and off again: refused as an unflagged handle is
        with pytest.raises(api.BossError, match="boss_kgp_set_grad"):
            gps[0].predict_grad(Xs[:, :3])
    finally:
        close_all(gps + [one])


# ------------------------------------------------------------------------------------------ set prediction
def member_moments(rows, Xs, mXs):
    """[S][P][M] moments, member by member (boss_gp_predict)."""
    mv = [[g.predict(Xs, mXs) for g in row] for row in rows]
    return np.array([[m for m, _ in row] for row in mv]), np.array([[v for _, v in row] for row in mv])


def second_output(X):
    return 0.4 + 0.3 * np.cos(3.0 * X.sum(0) / X.shape[0])


def restated_output(case, s, p):
    """The restatement of output p (0: the case's y, 1: second_output) at parameter set s, computed once."""
    if p == 0:
        return restated(case, s)
    key = (case, s, p)
    if key not in _restated:
        X, _, Xs, lam, amp, sig, disc, mX, mXs = setup(case)
        _restated[key] = cases.Restated(CLOSURES[CASES[case]["name"]], X, second_output(X), lam[:, s], amp[s], sig[s], Xs, disc, mX, mXs)
    return _restated[key]


@pytest.mark.parametrize("M", [1, M_MAX])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_acq_ei_over_a_fitted_set_takes_the_set_launches(B, api, case, P, M, monkeypatch):
    """S = 3 members (× P = 2 outputs, each output one boss_kgp_fit_batch call): one set of launches — _set_launches() rises, both
    counters, once per call —, while member-by-member predictions and the same call over create + update handles leave it alone.
    Values: bit for bit the epilogue on the member-by-member moments (both routes share one arithmetic order); and,
    like the same call over create + update handles, within the bound of tests/test_gpu_kernel_program.py of the acquisition computed
    from the restatement's moments: with s the smallest posterior standard deviation, tol_μ = tol(1+max|μ|), tol_v = tol·max k(x*,x*),
    |Δacq| <= tol_μ + 0.4·tol_v/(2s) + max E · (0.4·tol_μ/s + 0.242·tol_v/(2s²))."""
    from oracle import gp_oracle as O
    X, y, Xs, lam, amp, sig, disc, mX, mXs = setup(case)
    Xs = np.asfortranarray(Xs[:, :M])
    mXs = None if mXs is None else mXs[:M]
    S = 3
    Y = [y, second_output(X)][:P]
    coefs, y_max = [1.0, 0.0][:P], [np.inf, 0.5][:P]
    best = float(y.max())
    outs, ones = [], []
    cand = api.Candidates(Xs)
    try:
        for p in range(P):
            gps, _, st = api.kgp_fit_batch(X, Y[p], program(B, case), lam[:, :S], amp[:S], sig[:S], mX, disc)
            outs.append(gps)
            assert not st.any()
        rows = [[outs[p][s] for p in range(P)] for s in range(S)]
        means = None if mXs is None else np.broadcast_to(mXs, (S, P, M))
        a0, p0 = api._set_launches()
        acq, am, mx = api.acq_ei(rows, cand, coefs, y_max, best, mean_Xs=means)
        a1, p1 = api._set_launches()
        assert (a1 - a0, p1 - p0) == (1, 1)
        acq2, am2, mx2 = api.acq_ei(rows, cand, coefs, y_max, best, mean_Xs=means)
        _, am3, mx3 = api.acq_ei(rows, cand, coefs, y_max, best, mean_Xs=means, want_acq=False)
        assert np.array_equal(acq, acq2) and (am2, mx2) == (am, mx) and (am3, mx3) == (am, mx)
        a2 = api._set_launches()
        mu, var = member_moments(rows, Xs, mXs)
        acq_m, am_m, mx_m = api.acq_ei_moments(mu, var, coefs, y_max, best)
        print(f"[kprog set] {case} P={P} M={M}: max|acq - moments route| {np.abs(acq - acq_m).max():.3e}, argmax {am} / {am_m}")
        assert np.array_equal(acq, acq_m) and am == am_m and mx == mx_m and mx == acq[am]
        for s in range(S):
            ones.append([single(B, case, s, Y[p]) for p in range(P)])
        acq_1, am_1, mx_1 = api.acq_ei(ones, cand, coefs, y_max, best, mean_Xs=means)
        assert api._set_launches() == a2                      # member by member, and the singles: no set launch
        refs = [[restated_output(case, s, p) for p in range(P)] for s in range(S)]
        clip = lambda r: np.where((r.var[:M] < 0) & (r.var[:M] >= -1e-8), 0.0, r.var[:M])
        moments = {s: (np.stack([r.mu[:M] for r in refs[s]]), np.stack([clip(r) for r in refs[s]])) for s in range(S)}
        monkeypatch.setattr(O, "model_mean_and_var", lambda posts, Xs_, means_s=None: moments[posts[0]])
        want = O.ei_acquisition([[s] for s in range(S)], Xs, coefs, y_max, best)
        allr = [r for row in refs for r in row]
        tol = max(r.tol for r in allr)
        smin = min(np.sqrt(np.maximum(r.var[:M], 0.0)).min() for r in allr)
        tol_mu = tol * (1 + max(np.abs(r.mu[:M]).max() for r in allr))
        tol_v = tol * max(r.kss[:M].max() for r in allr)
        e_max = max(O.expected_improvement_lin(coefs, *moments[s], best).max() for s in range(S))
        bound = tol_mu + 0.4 * tol_v / (2 * smin) + e_max * (0.4 * tol_mu / smin + 0.242 * tol_v / (2 * smin * smin))
        print(f"[kprog set] {case} P={P} M={M}: max|acq - restatement| {np.abs(acq - want).max():.3e}, singles {np.abs(acq_1 - want).max():.3e}, "
              f"set - singles {np.abs(acq - acq_1).max():.3e} (bound {bound:.3e}, smin {smin:.3e})")
        assert max(r.cond for r in allr) < 1e6
        assert np.abs(acq - want).max() <= bound and np.abs(acq_1 - want).max() <= bound
        assert am == am_1 == int(np.argmax(want)) and mx == mx_1
    finally:
        cand.close()
        close_all([g for row in outs + ones for g in row])


def test_mixed_sets_go_member_by_member(B, api):
    """A built-in handle beside program handles, and two different programs: no set launch, and the values of the member-by-member
    moments under the same epilogue (within 2 ulp of the largest value: the mean over the samples is taken by another kernel)."""
    X, y, Xs, lam, amp, sig, _, _, _ = setup("dot3")
    cand = api.Candidates(Xs)
    S = 2
    gk, _, _ = api.kgp_fit_batch(X, y, program(B, "dot3"), lam[:, :S], amp[:S], sig[:S])
    ge, _, _ = api.kgp_fit_batch(X, y, kernel_of(B, "expo", 3).program, lam[:, :S], amp[:S], sig[:S])
    gb, _, _ = api.fit_batch(X, y, "matern52", lam[:, :S], amp[:S], sig[:S])
    try:
        for other in (gb, ge):
            rows = [[gk[s], other[s]] for s in range(S)]
            a0 = api._set_launches()
            acq, am, mx = api.acq_ei(rows, cand, [1.0, 0.0], [np.inf, 0.5], float(y.max()))
            assert api._set_launches() == a0
            acq2, am2, mx2 = api.acq_ei(rows, cand, [1.0, 0.0], [np.inf, 0.5], float(y.max()))
            assert np.array_equal(acq, acq2) and (am, mx) == (am2, mx2)
            mu, var = member_moments(rows, Xs, None)
            acq_m, am_m, _ = api.acq_ei_moments(mu, var, [1.0, 0.0], [np.inf, 0.5], float(y.max()))
            assert np.abs(acq - acq_m).max() <= 2 * np.finfo(float).eps * np.abs(acq_m).max() and am == am_m
    finally:
        cand.close()
        close_all(gk + ge + gb)


# ------------------------------------------------------------------------------------------ Python surface
def test_python_surface_over_two_samples_and_two_outputs(B, api):
    """model_posterior(list), HipBatchedMAP and HipBatchAM over BI samples of a two-output DeviceKernel model against the loop path of
    the previous routing, computed here from single handles: create + update per sample (model_posterior of one parameter set),
    one update per sample and output (data_loglike), the epilogue on member-by-member moments."""
    rng = np.random.default_rng(31)
    d, N, P = 2, 70, 2
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3.0 * X[0]) + np.cos(2.0 * X[1]), 0.3 * np.cos(3.0 * X.sum(0))])
    dk = kernel_of(B, "expo", d)
    pri = dict(lengthscale_priors=[B.MvLogNormal(np.log([0.5, 0.5]), [0.2, 0.2])] * P, amplitude_priors=[B.LogNormal(0.0, 0.2)] * P,
               noise_std_priors=[B.Dirac(0.05)] * P)
    model = B.HipGaussianProcess(kernel=dk, **pri)
    f = lambda x: [np.sin(3.0 * x[0]) + np.cos(2.0 * x[1]), 0.3 * np.cos(3.0 * x.sum())]
    prob = B.BossProblem(f, B.Domain(([0.0, 0.0], [1.0, 1.0])), B.ExpectedImprovement(B.LinFitness([1.0, 0.0])), model,
                         B.ExperimentData(X, Y), y_max=[np.inf, 0.5])
    sampler = model.params_sampler()
    r2 = np.random.default_rng(5)
    p1, p2 = sampler(r2), sampler(r2)
    Xs = np.asfortranarray(rng.uniform(0, 1, (d, 40)))
    posts = model.model_posterior([p1, p2], prob.data)
    loop = [model.model_posterior(p, prob.data) for p in (p1, p2)]
    try:
        for a, b in zip(posts, loop):
            assert isinstance(a.slices[0].gp, api.KernelGP)
            (mu, var), (mu1, var1) = a.mean_and_var(Xs), b.mean_and_var(Xs)
            assert mu.shape == (P, 40) and np.array_equal(mu, mu1) and np.array_equal(var, var1)
        # HipBatchedMAP: the first best of data_loglike + prior over its draws
        fitter = B.HipBatchedMAP(samples=6, seed=3)
        got = fitter.estimate_parameters(prob)
        draws_rng = np.random.default_rng(3)
        draws = [sampler(draws_rng) for _ in range(6)]
        ll = model.data_loglike(prob.data)
        vals = np.array([ll(p) + model.params_loglike()(p) for p in draws])
        for h in ll.handles:
            h.close()
        j = int(np.argmax(vals))
        assert got.loglike == vals[j] and np.array_equal(got.params.lengthscales, draws[j].lengthscales)
        assert np.array_equal(model.data_loglike_batch(prob.data, draws) + np.array([model.params_loglike()(p) for p in draws]), vals)
        # HipBatchAM over the two samples
        prob.params = [p1, p2]
        am = B.HipBatchAM(points=Xs)
        a0 = api._set_launches()[0]
        x, val = am.maximize_acquisition(prob)
        assert api._set_launches()[0] == a0 + 1
        _, acq = am.maximize_acquisition(prob, return_all=True)
        mv = [p.mean_and_var(Xs) for p in loop]
        from boss_jl_amd.maximizer import moments_acquisition
        acq_l, am_l, mx_l = moments_acquisition(prob, np.stack([m for m, _ in mv]), np.stack([v for _, v in mv]), Xs)
        assert np.array_equal(acq, acq_l) and np.array_equal(x, Xs[:, am_l]) and val == mx_l
    finally:
        for p in posts + loop:
            p.close()
    # a sample that is not positive definite raises as on the built-in path
    Xd = X.copy()
    Xd[:, 1] = Xd[:, 0]
    bad = B.HipGPParams(p1.lengthscales, p1.amplitudes, np.zeros(P))
    with pytest.raises(api.PosDefException, match="sample 1, output 0"):
        B.HipGaussianProcess(kernel=kernel_of(B, "dot1", d), **pri).model_posterior([p1, bad], B.ExperimentData(Xd, Y))


def test_python_surface_with_gradients_switched_on(B, api):
    """DeviceKernel(grad=True): the members of model_posterior(list) carry the flag (mean_and_var_grad equals the per-sample
    posterior's), and the scoring stage of HipSampleOptMAP — HipBatchedMAP(return_all=True) — scores as single updates do."""
    rng = np.random.default_rng(33)
    d, N = 2, 70
    X = rng.uniform(0, 1, (d, N))
    Y = (np.sin(3.0 * X[0]) + np.cos(2.0 * X[1]))[None, :]
    dk = B.DeviceKernel(cases.matern52, d, grad=True)
    model = B.HipGaussianProcess(kernel=dk, lengthscale_priors=[B.MvLogNormal(np.log([0.5, 0.5]), [0.2, 0.2])],
                                 amplitude_priors=[B.LogNormal(0.0, 0.2)], noise_std_priors=[B.Dirac(0.05)])
    prob = B.BossProblem(lambda x: [np.sin(3.0 * x[0]) + np.cos(2.0 * x[1])], B.Domain(([0.0, 0.0], [1.0, 1.0])),
                         B.ExpectedImprovement(B.LinFitness([1.0])), model, B.ExperimentData(X, Y))
    sampler = model.params_sampler()
    r2 = np.random.default_rng(6)
    plist = [sampler(r2) for _ in range(3)]
    Xs = np.asfortranarray(rng.uniform(0, 1, (d, 33)))
    posts = model.model_posterior(plist, prob.data)
    loop = [model.model_posterior(p, prob.data) for p in plist]
    try:
        for a, b in zip(posts, loop):
            for u, v in zip(a.mean_and_var_grad(Xs), b.mean_and_var_grad(Xs)):
                assert np.array_equal(u, v)
    finally:
        for p in posts + loop:
            p.close()
    scored = B.HipBatchedMAP(samples=5, seed=4).estimate_parameters(prob, return_all=True)
    ll = model.data_loglike(prob.data)
    want = [ll(m.params) + model.params_loglike()(m.params) for m in scored]
    for h in ll.handles:
        h.close()
    assert [m.loglike for m in scored] == want
    got = B.HipSampleOptMAP(5, 2, 2, seed=4).estimate_parameters(prob)
    assert np.isfinite(got.loglike)


if __name__ == "__main__":                                    # the child of test_chunks_agree_bitwise_with_one_batch
    entry.build()
    import boss_jl_amd as B_
    ll_, st_ = chunk_call(B_.api, B_)
    np.savez(sys.argv[1], ll=ll_, st=st_)
