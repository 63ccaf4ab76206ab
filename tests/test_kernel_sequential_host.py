"""Host-side checks of the opt-in appends / tracked candidates of program-kernel posteriors (boss_kgp_set_sequential,
B.DeviceKernel(f, x_dim, sequential=True)); no GPU needed: the symbol is declared, exported and mirrored, a NULL handle is refused
without a device, the Python switch travels with the kernel object and decides what refuse_device_kernel lets through,
HipSequentialBatchAM checks its arguments before it touches the library and closes everything it opened when a pick raises, and the
kernels this adds or re-templates use no scratch memory."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_program_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "boss_kgp_set_sequential"


def test_the_switch_is_declared_exported_and_mirrored():
    from boss_jl_amd import api
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "bosship.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*boss_gp_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)" % SYM, hdr)
    assert hasattr(lib, SYM) and SYM in api.SIGNATURES
    assert api.SIGNATURES[SYM] == api.SIGNATURES["boss_kgp_set_grad"]
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert SYM in open(os.path.join(ROOT, doc)).read(), doc
    import inspect
    assert inspect.signature(api.KernelGP.__init__).parameters["sequential"].default is False
    assert inspect.signature(api.kgp_fit_batch).parameters["sequential"].default is False


def test_a_null_handle_is_refused_without_a_device():
    from boss_jl_amd import api
    lib = api.load_library()
    for on in (0, 1):
        assert getattr(lib, SYM)(None, on) == api.BOSS_E_INVALID
        assert b"NULL" in lib.boss_last_error()


def _model(B, kernel, **kw):
    return B.HipGaussianProcess(lengthscale_priors=[None], amplitude_priors=[None], noise_std_priors=[None], kernel=kernel, **kw)


def test_the_python_switch_travels_with_the_kernel():
    import boss_jl_amd as B
    from boss_jl_amd.kernel import device_kernel_of
    plain, seq = B.DeviceKernel(cases.expo, 2), B.DeviceKernel(cases.expo, 2, sequential=True)
    assert plain.sequential is False and seq.sequential is True and seq.grad is False
    both = B.DeviceKernel(cases.sqexp, 2, grad=True, sequential=True)
    assert both.grad and both.sequential
    assert np.array_equal(seq.program.code, plain.program.code)          # the flag changes nothing of the traced program
    m = _model(B, seq).make_discrete([False, True])
    assert device_kernel_of(m) is seq and device_kernel_of(m).sequential and list(m.discrete) == [False, True]


def test_refuse_device_kernel_knows_the_switch():
    import boss_jl_amd as B
    from boss_jl_amd.kernel import refuse_device_kernel
    plain, seq = _model(B, B.DeviceKernel(cases.expo, 2)), _model(B, B.DeviceKernel(cases.expo, 2, sequential=True))
    builtin = _model(B, "matern52")
    for what in ("append", "HipSequentialBatchAM (appending observations, tracked candidates)"):
        with pytest.raises(NotImplementedError, match="DeviceKernel") as e:
            refuse_device_kernel(plain, what, seq_ok=True)
        assert "DeviceKernel(f, x_dim, sequential=True) switches appends and tracked candidates on" in str(e.value) and what in str(e.value)
        with pytest.raises(NotImplementedError, match="DeviceKernel"):
            refuse_device_kernel(plain, what)
        refuse_device_kernel(seq, what, seq_ok=True)             # a flagged kernel passes
        refuse_device_kernel(builtin, what, seq_ok=True)
    for m in (plain, seq):                                       # covariances stay refused, flagged or not
        with pytest.raises(NotImplementedError, match="DeviceKernel"):
            refuse_device_kernel(m, "cov / mean_and_cov")
    with pytest.raises(NotImplementedError, match="grad=True"):  # the two switches are independent
        refuse_device_kernel(seq, "mean_and_var_grad", grad_ok=True)
    with pytest.raises(NotImplementedError, match="sequential=True"):
        refuse_device_kernel(_model(B, B.DeviceKernel(cases.sqexp, 2, grad=True)), "append", seq_ok=True)


# ------------------------------------------------------------------------------------------ HipSequentialBatchAM on fakes
class Untouchable:
    def __getattr__(self, name):
        raise AssertionError("the library was touched: " + name)


def _problem(B, kernel, N=6):
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (2, N))
    prm = B.HipGPParams(np.full((2, 1), 0.5), [1.0], [0.1])
    return B.BossProblem(None, B.Domain((np.zeros(2), np.ones(2))), B.ExpectedImprovement(B.LinFitness([1.0])), _model(B, kernel),
                         B.ExperimentData(X, X.sum(0)[None, :]), [np.inf], prm)


def test_sequential_batch_checks_its_arguments_first(monkeypatch):
    import boss_jl_amd as B
    from boss_jl_amd import api
    prob = _problem(B, B.DeviceKernel(cases.expo, 2))            # (tracing checks the program with the library's host interpreter)
    monkeypatch.setattr(api, "load_library", lambda path=None: Untouchable())
    pts = np.zeros((2, 4))
    with pytest.raises(NotImplementedError, match="sequential=True"):
        B.HipSequentialBatchAM(B.HipBatchAM(points=pts), 2).maximize_acquisition(prob)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="batch_size"):
            B.HipSequentialBatchAM(B.HipBatchAM(points=pts), bad).maximize_acquisition(_problem(B, "matern52"))


class FakeGP:
    device = 0


class FakeSlice:
    def __init__(self, log, name):
        self.log, self.name, self.gp = log, name, FakeGP()

    def _mean_s(self, X):
        return None


class FakePost:
    def __init__(self, log, name, fail=False):
        self.log, self.name, self.fail, self.closed = log, name, fail, False
        self.slices = [FakeSlice(log, name + "p0")]

    def mean(self, x):
        return np.zeros(1)

    def append(self, x, y):
        if self.fail:
            raise RuntimeError("no append")
        self.log.append(("append", self.name))

    def close(self):
        self.closed = True
        self.log.append(("post.close", self.name))


@pytest.mark.parametrize("route", ["tracked", "untracked"])
def test_sequential_batch_closes_everything_when_a_pick_raises(monkeypatch, route):
    import boss_jl_amd as B
    from boss_jl_amd import api, maximizer
    log, made = [], []

    class Cand:
        def __init__(self, Xs, dev=0):
            self.M, self.closed = Xs.shape[1], False
            made.append(self)

        def close(self):
            self.closed = True

    class Track:
        def __init__(self, gp, cand, mean_Xs=None):
            self.closed = False
            made.append(self)

        def moments(self, first=0, count=None):
            return np.zeros(1), np.ones(1)

        def close(self):
            self.closed = True
    posts = [FakePost(log, "s0"), FakePost(log, "s1", fail=True)]
    monkeypatch.setattr(api, "load_library", lambda path=None: Untouchable())
    monkeypatch.setattr(api, "Candidates", Cand)
    monkeypatch.setattr(api, "Track", Track)
    monkeypatch.setattr(api, "acq_ei_tracks", lambda tracks, *a, **k: (None, 1, 0.5))
    monkeypatch.setattr(maximizer, "posteriors_of", lambda prob, lo=None, hi=None, reserve=0: log.append(("reserve", reserve)) or posts)
    prob = _problem(B, "matern52")
    pts = np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (2, 5)))
    am = B.HipBatchAM(points=pts) if route == "tracked" else B.HipBatchAM(points=pts, shard="outputs")
    if route == "untracked":
        monkeypatch.setattr(B.HipBatchAM, "maximize_acquisition", lambda self, prob, options=None, posts=None: (pts[:, 1].copy(), 0.5))
    with pytest.raises(RuntimeError, match="no append"):
        B.HipSequentialBatchAM(am, 3).maximize_acquisition(prob)
    assert log[0] == ("reserve", 3) and ("append", "s0") in log
    assert all(p.closed for p in posts)
    if route == "tracked":
        assert len(made) == 1 + 2 and all(x.closed for x in made)   # the candidate buffer and one track per sample
    else:
        assert made == []
    assert prob.data.X.shape[1] == 6                             # the caller's problem is untouched


# ------------------------------------------------------------------------------------------ the kernels
def test_the_sequential_kernels_use_no_scratch(tmp_path):
    """kprog_track_rhs_kernel and kprog_col_kernel (new), both instantiations of track_append_kernel, the Gram and K* kernels the
    appends and tracks launch and append_scalars_kernel: private_segment_fixed_size = 0 in the code object's metadata (the check of tests/test_cov_models_host.py)."""
    out = tmp_path / "bosship.s"
    flags = [f for f in entry.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags +
                          ["-S", "--cuda-device-only", "-o", str(out), os.path.join(entry.CSRC, "bosship.hip")])
    txt = out.read_text()
    want = ("kprog_track_rhs_kernel", "kprog_col_kernel", "track_append_kernel", "kprog_gram_kernel", "kprog_kstar_kernel", "append_scalars_kernel")
    found = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", txt, re.S):
        name, scratch = m.group(2), int(m.group(3))
        for k in want:
            if k in name and "gibbs" not in name and "aug_" not in name:
                found.setdefault(k, set()).add(name)
                assert scratch == 0, (name, scratch)
    assert set(found) == set(want), found
    assert len(found["track_append_kernel"]) == 2 and len(found["kprog_kstar_kernel"]) == 2, found
