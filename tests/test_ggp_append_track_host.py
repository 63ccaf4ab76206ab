"""Host-side checks of the gradient-observation append / reserve / tracked-candidates entry points (no GPU): the header, the Julia
glue and INTEGRATION.md name them, the Python wrappers lay their arguments out as the ABI takes them (a fake library records the
calls), B.gradient_sequential_batch runs its reserve / track / select / append / close sequence with the documented speculative
observation, and the two index maps of the handle's mixed row ordering (restated here) are what the design says they are."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("boss_ggp_reserve", "boss_ggp_track_create")


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
    assert len(api.SIGNATURES["boss_ggp_reserve"][1]) == 2 and len(api.SIGNATURES["boss_ggp_track_create"][1]) == 3
    assert issubclass(api.GradTrack, api.Track) and api.GradGP.reserve is not api.GP.reserve
    # the header says what the append now does, and nobody claims a rebuild any more
    full = read("include", "bosship.h")
    blk = full[full.index("/* augment_dataset! (src/types/problem.jl:191-198) + the posterior at unchanged hyper-parameters: n_new"):]
    blk = blk[:blk.index("int boss_ggp_append(")]
    assert "only the 128-row blocks that contain new rows are rebuilt" in blk and "verbatim" in blk
    assert "rebuilt and factorised again" not in blk
    src = read("boss.jl_amd", "csrc", "host_factor.inc") + read("boss.jl_amd", "csrc", "host_append.inc")
    assert "replace_with_rebuilt" not in src and "hipMemcpyDeviceToHost, c->stream));\n        HIPCHK(hipMemcpyAsync(yt.data()" not in src
    for path in (("boss.jl_amd", "api.py"), ("boss.jl_amd", "gradient_gp.py"), ("README.md",), ("INTEGRATION.md",)):
        txt = read(*path)
        assert "the augmented system is rebuilt and factorised" not in txt and "rebuilt and re-factorised" not in txt, path
    design = read("DESIGN.md")
    assert "append still rebuilds" not in design and "tracked candidates of the gradient-observation model" not in design


# ------------------------------------------------------------------------------------------ a fake library
class FakeLib:
    """Records every call; fills the out-parameters the wrappers read."""

    def __init__(self):
        self.calls = []
        self.rows = 0
        self.rc = 0

    def boss_last_error(self):
        return b"fake"

    def boss_ggp_reserve(self, h, n):
        self.calls.append(("boss_ggp_reserve", h, n))
        return 0

    def boss_ggp_append(self, h, m, X, y, dY, out):
        d = self.d
        self.calls.append(("boss_ggp_append", h, m, np.ctypeslib.as_array(X, (d * m,)).copy(), np.ctypeslib.as_array(y, (m,)).copy(),
                           np.ctypeslib.as_array(dY, (d * m,)).copy()))
        self.rows += m * (1 + d)
        out._obj.value = -12.5
        return self.rc

    def boss_gp_n(self, h, out):
        out._obj.value = self.rows
        return 0

    def boss_ggp_track_create(self, gp, cand, out):
        self.calls.append(("boss_ggp_track_create", gp, cand))
        out._obj.value = 77
        return 0

    def boss_track_free(self, h):
        self.calls.append(("boss_track_free", h.value if hasattr(h, "value") else h))


class FakeCand:
    d, M, _h = 3, 5, 21


def fake_handle(api, d=3, n=5):
    g = object.__new__(api.GradGP)
    g.d, g.n, g.N, g._h, g.logpdf = d, n, n * (1 + d), 11, None
    return g


def test_argument_layout_of_the_new_calls(monkeypatch):
    from boss_jl_amd import api
    lib = FakeLib()
    lib.d, lib.rows = 3, 20
    monkeypatch.setattr(api, "load_library", lambda path=None: lib)
    g = fake_handle(api)
    with pytest.raises(api.BossError):                          # the positional count of GP.reserve (observations) stays refused
        g.reserve(9)
    with pytest.raises(api.BossError):
        g.reserve()
    assert lib.calls == []
    g.reserve(points=9)
    assert lib.calls == [("boss_ggp_reserve", 11, 9)]
    # append: X_new d×m and dY_new d×m column-major (point after point), y_new m
    X = np.arange(6.0).reshape(3, 2)
    dY = 10 + np.arange(6.0).reshape(3, 2)
    lp = g.append(X, [0.5, -0.5], dY)
    name, h, m, xb, yb, db = lib.calls[-1]
    assert (name, h, m) == ("boss_ggp_append", 11, 2) and lp == -12.5
    assert np.array_equal(xb, X.T.reshape(-1)) and np.array_equal(yb, [0.5, -0.5]) and np.array_equal(db, dY.T.reshape(-1))
    assert g.n == 7 and g.N == 28                               # read back from the handle (boss_gp_n counts rows)
    lib.rc = api.BOSS_E_NOT_PD                                  # a failed factorisation: the points are in the handle all the same
    with pytest.raises(api.PosDefException):
        g.append(X[:, :1], [0.1], dY[:, :1])
    assert g.n == 8 and g.N == 32
    with pytest.raises(ValueError):
        g.append(X, [0.5], dY)
    # the track
    tr = api.GradTrack(g, FakeCand())
    assert lib.calls[-1] == ("boss_ggp_track_create", 11, 21) and tr.M == 5 and tr.gp is g
    tr.close()
    assert lib.calls[-1] == ("boss_track_free", 77) and tr._h is None
    tr.close()                                                  # idempotent
    assert lib.calls[-1] == ("boss_track_free", 77) and sum(c[0] == "boss_track_free" for c in lib.calls) == 1
    g._h = None


# ------------------------------------------------------------------------------------------ the sequential batch
class FakeTrack:
    def __init__(self, log, name):
        self.log, self.name, self.closed = log, name, False

    def close(self):
        self.closed = True
        self.log.append(("track.close", self.name))


class FakeGP:
    device = 0


class FakeSlice:
    """mean_and_var_grad(x) = (a + sum(x), ·, b·ones, ·): distinct per slice, so the average is recognisable."""

    def __init__(self, log, name, a, b, fail=None):
        self.log, self.name, self.a, self.b, self.fail, self.gp = log, name, a, b, fail, FakeGP()

    def reserve(self, extra):
        self.log.append(("reserve", self.name, extra))

    def track(self, cand, Xs):
        if self.fail == "track":
            raise RuntimeError("no track")
        self.log.append(("track", self.name))
        t = FakeTrack(self.log, self.name)
        self.made = t
        return t

    def mean_and_var_grad(self, X):
        d = X.shape[0]
        return np.array([self.a + X.sum()]), np.zeros(1), np.full((d, 1), self.b), np.zeros((d, 1))

    def append(self, x, y, dy):
        if self.fail == "append":
            raise RuntimeError("no append")
        self.log.append(("append", self.name, x.copy(), float(y), np.array(dy, float).copy()))


def fake_env(monkeypatch, log, picks):
    from boss_jl_amd import api

    class Cand:
        def __init__(self, Xs, dev):
            log.append(("cand", Xs.shape, dev))
            self.closed = False

        def close(self):
            self.closed = True
            log.append(("cand.close",))
    it = iter(picks)

    def acq_ei_tracks(tracks, coefs, y_max, best, valid_mask, want_acq=True):
        log.append(("select", [[t.name for t in row] for row in tracks], best, want_acq))
        return None, next(it), 0.0
    monkeypatch.setattr(api, "Candidates", Cand)
    monkeypatch.setattr(api, "acq_ei_tracks", acq_ei_tracks)


def test_sequential_batch_sequence_and_speculative_rule(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import gradient_gp
    assert B.gradient_sequential_batch is gradient_gp.gradient_sequential_batch
    doc = gradient_gp.gradient_sequential_batch.__doc__
    assert "cannot run on GradientData" in doc and "batch.jl:32-37" in doc and "gradient_data.jl:47-53" in doc
    log = []
    fake_env(monkeypatch, log, [2, 0])
    d, M = 3, 4
    Xs = np.arange(12.0).reshape(d, M) / 10
    posts = [[FakeSlice(log, "s0p0", 1.0, 0.5), FakeSlice(log, "s0p1", -1.0, 2.0)],
             [FakeSlice(log, "s1p0", 3.0, 1.5), FakeSlice(log, "s1p1", -2.0, 4.0)]]
    Y = np.array([[0.1, 0.7], [0.0, 0.2]])
    sel = gradient_gp.gradient_sequential_batch(posts, Xs, 2, [1.0, 0.0], [np.inf, 0.45], Y)
    assert np.array_equal(sel, Xs[:, [2, 0]])
    names = [e[0] for e in log]
    # reserve everything first, then the tracks, then select / append alternate, everything closed at the end
    assert names[:9] == ["cand"] + ["reserve"] * 4 + ["track"] * 4
    assert all(e[2] == 2 for e in log[1:5])
    assert names[9:19] == ["select"] + ["append"] * 4 + ["select"] + ["append"] * 4
    assert names[19:] == ["track.close"] * 4 + ["cand.close"]
    assert log[9][1] == [["s0p0", "s0p1"], ["s1p0", "s1p1"]] and log[9][3] is False
    assert log[9][2] == 0.7                                     # best so far of output 0 among the feasible observations
    # the speculative observation: the sample-averaged mean and mean gradient at the selected point, the same for every sample
    x = Xs[:, 2]
    for e in log[10:14]:
        i = int(e[1][-1])
        assert np.array_equal(e[2], x)
        assert e[3] == pytest.approx(((1.0, -1.0)[i] + (3.0, -2.0)[i]) / 2 + x.sum(), abs=1e-15)
        assert np.allclose(e[4], np.full(d, ((0.5, 2.0)[i] + (1.5, 4.0)[i]) / 2), rtol=0, atol=1e-15)
    assert log[14][2] == pytest.approx(max(0.7, 2.0 + x.sum()))    # the incumbent grows with the speculative value


@pytest.mark.parametrize("fail", ["track", "append"])
def test_sequential_batch_closes_everything_on_an_exception(monkeypatch, fail):
    from boss_jl_amd import gradient_gp
    log = []
    fake_env(monkeypatch, log, [1])
    Xs = np.zeros((2, 3))
    posts = [[FakeSlice(log, "a", 0.0, 0.0), FakeSlice(log, "b", 0.0, 0.0, fail=fail)]]
    with pytest.raises(RuntimeError):
        gradient_gp.gradient_sequential_batch(posts, Xs, 1, [1.0, 0.0])
    assert posts[0][0].made.closed and log[-1] == ("cand.close",)
    if fail == "append":
        assert posts[0][1].made.closed


def test_sequential_batch_checks_its_arguments_first(monkeypatch):
    from boss_jl_amd import api, gradient_gp

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the library was touched: " + name)
    monkeypatch.setattr(api, "load_library", lambda path=None: Untouchable())
    Xs = np.zeros((3, 4))
    with pytest.raises(ValueError):
        gradient_gp.gradient_sequential_batch([[object()]], Xs, 0, [1.0])
    with pytest.raises(ValueError):
        gradient_gp.gradient_sequential_batch([], Xs, 2, [1.0])
    with pytest.raises(ValueError):
        gradient_gp.gradient_sequential_batch([[]], Xs, 2, [1.0])
    assert callable(gradient_gp.HipGradientGPPosteriorSlice.track) and callable(gradient_gp.HipGradientGPPosteriorSlice.reserve)
    assert "rebuilt" not in gradient_gp.HipGradientGPPosteriorSlice.append.__doc__


# ------------------------------------------------------------------------------------------ the index maps
def row_of(l, pt, nhead, d):
    """(component l, point) -> row: the head keeps the reference's component-major rows, a later point owns 1 + d rows in a run."""
    return l * nhead + pt if pt < nhead else nhead * (1 + d) + (pt - nhead) * (1 + d) + l


def decode(row, nhead, d):
    """row -> (l, point)."""
    if row < nhead * (1 + d):
        return row // nhead, row % nhead
    q = row - nhead * (1 + d)
    return q % (1 + d), nhead + q // (1 + d)


MAP_CASES = [(3, 5, 10), (3, 31, 32), (3, 32, 33), (3, 63, 66), (3, 127, 130), (3, 10, 70), (1, 250, 260), (8, 56, 58), (16, 30, 32),
             (3, 50, 70), (16, 1, 3)]


@pytest.mark.parametrize("d,nhead,npts", MAP_CASES)
def test_index_maps(d, nhead, npts):
    N = npts * (1 + d)
    rows = [row_of(l, pt, nhead, d) for pt in range(npts) for l in range(1 + d)]
    assert sorted(rows) == list(range(N))                       # a permutation of 0 … N−1
    for row in range(N):
        l, pt = decode(row, nhead, d)
        assert 0 <= l <= d and 0 <= pt < npts and row_of(l, pt, nhead, d) == row     # inverse to each other
    for pt in range(npts):
        for l in range(1 + d):
            assert decode(row_of(l, pt, nhead, d), nhead, d) == (l, pt)
    # never appended to: the reference's ordering [y; ∂₁y; …; ∂_d y]
    assert all(row_of(l, pt, npts, d) == l * npts + pt for pt in range(npts) for l in range(1 + d))
    assert all(decode(r, npts, d) == (r // npts, r % npts) for r in range(N))
    # an append only adds rows at the end: the rows of the first npts − 1 points do not depend on the last one
    assert all(row_of(l, pt, nhead, d) < (npts - 1) * (1 + d) for pt in range(npts - 1) for l in range(1 + d))
    # the device code's closed form of a later point's rows (gram_kernels.hpp: pt (1 + d) + l)
    assert all(row_of(l, pt, nhead, d) == pt * (1 + d) + l for pt in range(nhead, npts) for l in range(1 + d))
    src = read("boss.jl_amd", "csrc", "gram_kernels.hpp")
    assert "aug_row_decode" in src and "aug_row_of" in src
