"""What tests/test_acq_program_host.py and tests/test_gpu_acq_program.py share: the closures, the branch-free spelling of
EI × feasibility as an acquisition program with a numpy restatement of it and of its reverse sweep (independent of the C
interpreter), the selection of fixture groups (tests/golden/acq_tails.json, tests/acq_tails_cases.py) the spelling is pinned on,
and the workgroup shapes of the two kernels.

ei_fp(coefs) spells the built-in acquisition branch-free over q = [best, y_max_1..P]:
    muf = c_1 μ_1 + … (sequential),  vf = c_1² σ²_1 + … (sequential),  sf = sqrt(vf),  diff = muf − best,  z = diff/sf,
    value = (diff·Φ(z) + sf·φ(z)) · Π_p Φ((y_max_p − μ_p)/sqrt(σ²_p))        (has_best=False: the product alone)
The coefficients are traced constants.  An output without a constraint has y_max = +Inf: its factor is Φ(+Inf) = 1 exactly.  The
spelling has none of ei_value's branches (σ = 0 with y_max = μ, diff = 0 with sf = 0), so it is pinned only where they are not taken.

Fixture groups the spelling is pinned on (the rule of value_groups / grad_groups below): not a twin, P <= 8, check != "tiny", every
variance > 0, vf > 0, and not the "no best, no y_max" mode.  Today: 24 value groups, 2077 candidates.  Worst err/(u·cond) of the numpy
restatement over them, measured on a CPU (the fixture's device_C is 16 for values and for gradients):
    values      2.01  (at fp-1)
    gradients   g-tail-d1 2.55, g-tail-d3 2.28, and of the further gradient groups those on which the numpy reverse sweep stays
                within device_C/4 = 4: g-ei-p2 0.708, g-ei-p3 0.754, g-fp-1 2.14, g-fp-2 1.90, g-eifp 0.832 — all five selectable
                ones (GRAD_GROUPS below); the CPU decided before any device run.
"""
import numpy as np

import acq_tails_cases as T
import boss_jl_amd as B

U = T.U


# ------------------------------------------------------------------------------------------ closures
def ucb(c, beta):
    c = np.asarray(c, dtype=np.float64)
    return lambda mu, var, q: mu @ c + beta * np.sqrt(var @ (c * c))


def pi(c, xi=0.0):
    """Probability of improvement × feasibility; q = [best, y_max_1..P]."""
    c = np.asarray(c, dtype=np.float64)

    def closure(mu, var, q):
        a = B.normcdf((mu @ c - q[0] - xi) / np.sqrt(var @ (c * c)))
        for p in range(len(c)):
            a = a * B.normcdf((q[1 + p] - mu[p]) / np.sqrt(var[p]))
        return a
    return closure


def max_variance(mu, var, q):
    return var.sum()


def clamp(mu, var, q):
    """np.minimum / np.maximum: P = 2, Q = 1."""
    return np.minimum(np.maximum(mu[0] - q[0], 0.25 * mu[1]), var.sum())


def long_minmax(mu, var, q):
    """A program near the instruction limit (P = 3, Q = 4): the value kernel runs it with one wave per workgroup."""
    a = q[3]
    for p in range(3):
        for k in range(3):
            a = a + np.minimum(mu[p] * q[k], np.sqrt(var[p])) * np.maximum(mu[p], q[k] - var[p])
    return a


def ei_fp(coefs, has_best=True):
    c = [float(t) for t in np.asarray(coefs, dtype=np.float64).reshape(-1)]
    P = len(c)

    def closure(mu, var, q):
        a = None
        if has_best:
            muf, vf = c[0] * mu[0], (c[0] * c[0]) * var[0]
            for p in range(1, P):
                muf, vf = muf + c[p] * mu[p], vf + (c[p] * c[p]) * var[p]
            sf, diff = np.sqrt(vf), muf - q[0]
            z = diff / sf
            a = diff * B.normcdf(z) + sf * B.normpdf(z)
        for p in range(P):
            f = B.normcdf((q[1 + p] - mu[p]) / np.sqrt(var[p]))
            a = f if a is None else a * f
        return a
    return closure


def ei_fp_q(P, best, y_max):
    return np.concatenate([[0.0 if best is None else best], np.full(P, np.inf) if y_max is None else np.asarray(y_max, float)])


def ei_fp_acquisition(coefs, has_best=True):
    """DeviceAcquisition(ei_fp) whose scalars come from the problem as ExpectedImprovement's do."""
    P = len(coefs)
    fit = B.LinFitness(coefs)

    def params(problem):
        from boss_jl_amd.problem import best_so_far
        return ei_fp_q(P, best_so_far(fit, problem.data.Y, problem.y_max), problem.y_max)
    return B.DeviceAcquisition(ei_fp(coefs, has_best), P, n_params=1 + P, params=params, outside=0.0)


# name -> (closure, P, Q); the programs are traced once per process (programs())
CLOSURES = {
    "ucb": (ucb([1.0, -0.5], 2.0), 2, 0),
    "ucb1": (ucb([1.0], 1.5), 1, 0),
    "pi": (pi([1.0, 0.5, -0.25], 0.01), 3, 4),
    "pi1": (pi([1.0]), 1, 2),
    "max_variance": (max_variance, 3, 0),
    "clamp": (clamp, 2, 1),
    "long_minmax": (long_minmax, 3, 4),
    "ei_fp1": (ei_fp([1.0]), 1, 2),
    "ei_fp2": (ei_fp([1.0, -0.5]), 2, 3),
    "ei_fp3": (ei_fp([0.7, 0.2, -1.1]), 3, 4),
}
_programs = {}


def programs():
    if not _programs:
        for name, (f, P, Q) in CLOSURES.items():
            _programs[name] = B.trace_acquisition(f, P, Q)
    return _programs


def waves(prog, grad):
    """Waves per workgroup of the value / gradient kernel for a program: acqp_block of csrc/host_acqprog.inc (as many of 4 as fit
    64 KiB; a thread's column is 2P + Q + nI doubles, twice that with the adjoints)."""
    slots = (2 if grad else 1) * (2 * prog.y_dim + prog.n_params + prog.code.shape[0])
    return max(1, min(4, (64 * 1024) // (8 * 64 * slots)))


# ------------------------------------------------------------------------------------------ numpy restatement of ei_fp
def _ncdf(z):
    from scipy.special import erfc
    return 0.5 * erfc(-z * 0.7071067811865476)


def _npdf(z):
    return np.exp(-0.5 * z * z) * 0.3989422804014327


def ei_fp_numpy(coefs, has_best, mu, var, q, want_grad=False):
    """value[M] (and ∂value/∂μ[P, M], ∂value/∂σ²[P, M]) of the spelling at moments mu, var [P, M]: plain numpy, the adjoints written
    out by hand in the order a reverse sweep visits them."""
    c = np.asarray(coefs, dtype=np.float64)
    P, M = mu.shape
    with np.errstate(all="ignore"):
        s = np.sqrt(var)
        t = (np.asarray(q[1:1 + P])[:, None] - mu) / s
        F = _ncdf(t)
        if has_best:
            muf, vf = c[0] * mu[0], (c[0] * c[0]) * var[0]
            for p in range(1, P):
                muf, vf = muf + c[p] * mu[p], vf + (c[p] * c[p]) * var[p]
            sf, diff = np.sqrt(vf), muf - q[0]
            z = diff / sf
            Phi, phi = _ncdf(z), _npdf(z)
            ei = diff * Phi + sf * phi
            pre = [ei]
        else:
            pre = [F[0]]
        for p in range(0 if has_best else 1, P):
            pre.append(pre[-1] * F[p])
        val = pre[-1]
        if not want_grad:
            return val
        # adjoints of the product chain, last factor first
        aF = np.zeros((P, M))
        w = np.ones(M)
        first = 0 if has_best else 1
        for p in range(P - 1, first - 1, -1):
            aF[p] = w * pre[p - first]
            w = w * F[p]
        if has_best:
            a_ei = w
        else:
            aF[0] = w
        a_t = np.where(aF == 0.0, 0.0, aF * _npdf(t))
        a_mu = np.where(a_t == 0.0, 0.0, -a_t / s)
        a_s = np.where(a_t == 0.0, 0.0, a_t * (-t / s))
        a_var = np.where(a_s == 0.0, 0.0, a_s * (0.5 / s))
        if has_best:
            a_z = a_ei * diff * phi + a_ei * sf * (-z * phi)
            a_diff = a_ei * Phi + a_z / sf
            a_sf = a_ei * phi + a_z * (-z / sf)
            a_vf = a_sf * (0.5 / sf)
            a_mu = a_mu + c[:, None] * a_diff[None, :]
            a_var = a_var + (c * c)[:, None] * a_vf[None, :]
    return val, a_mu, a_var


def fold(a_mu, a_var, var, dmu, dvar):
    """Σ_p (ā_μp ∂μ_p + ā_vp ∂σ²_p) per coordinate: a_mu, a_var, var [P, M]; dmu, dvar [P, d, M] -> [d, M].  An output whose variance
    is <= 0 has no σ² term."""
    g = np.zeros(dmu.shape[1:])
    for p in range(dmu.shape[0]):
        g = g + a_mu[p][None, :] * dmu[p]
        g = g + np.where((var[p] > 0)[None, :], a_var[p][None, :] * dvar[p], 0.0)
    return g


def group_numpy(g, want_grad=False):
    """The numpy restatement on a fixture group: samples added in ascending order, scaled by 1/S once."""
    has_best = g["best"] is not None
    coefs = g["coefs"] if has_best else np.zeros(g["P"])
    q = ei_fp_q(g["P"], g["best"], g["y_max"])
    if want_grad:
        val, a_mu, a_var = ei_fp_numpy(coefs, has_best, g["mu"][0], g["var"][0], q, True)
        return val, fold(a_mu, a_var, g["var"][0], g["dmu"], g["dvar"])
    acc = None
    for s in range(g["S"]):
        a = ei_fp_numpy(coefs, has_best, g["mu"][s], g["var"][s], q)
        acc = a if acc is None else acc + a
    return acc * (1.0 / g["S"]) if g["S"] > 1 else acc


# ------------------------------------------------------------------------------------------ fixture groups
def _selectable(g):
    if g["twin"] or g["P"] > 8 or g["check"] == "tiny" or not np.all(g["var"] > 0):
        return False
    if g["best"] is None and g["y_max"] is None:
        return False
    if g["best"] is not None:
        c = g["coefs"]
        if not np.all(np.einsum("p,spm->sm", c * c, g["var"]) > 0):
            return False
    return True


def value_groups():
    return [g for g in T.load()["groups"] if g["kind"] == "value" and _selectable(g)]


# Gradient groups: the two tail groups, and the further selectable ones on which the numpy reverse sweep stays within device_C/4 = 4
# (measured err/(u·gcond), worst coordinate and candidate).  test_acq_program_host.py re-measures and asserts the list.
GRAD_GROUPS = {"g-tail-d1": 2.55, "g-tail-d3": 2.28, "g-ei-p2": 0.708, "g-ei-p3": 0.754, "g-fp-1": 2.14, "g-fp-2": 1.90, "g-eifp": 0.832}


def grad_candidates():
    return [g for g in T.load()["groups"] if g["kind"] == "grad" and _selectable(g)]


def grad_groups():
    by = T.load()["by_name"]
    return [by[n] for n in GRAD_GROUPS]


_group_programs = {}


def group_program(g):
    """The traced ei_fp program of a fixture group and its scalars."""
    has_best = g["best"] is not None
    coefs = g["coefs"] if has_best else np.zeros(g["P"])
    key = (tuple(coefs), has_best)
    if key not in _group_programs:
        _group_programs[key] = B.trace_acquisition(ei_fp(coefs, has_best), g["P"], 1 + g["P"])
    return _group_programs[key], ei_fp_q(g["P"], g["best"], g["y_max"])


# ------------------------------------------------------------------------------------------ bars between two device paths
def ei_fp_cond(O, coefs, mu, var, best, y_max):
    """acq_truth's first-order condition sum of EI × feasibility in fp64 for P outputs (mu, var [P, M]): the P > 1 analogue of
    acq_tails_cases.ei_cond_fp64.  EI: (1+z²)(|T1|+|T2|) + P·Φ(z)(Σ|c_p μ_p| + |b|);  FP: FP·Σ_p(1+t_p²) over the finite t_p;
    EI·FP: cond_EI·FP + |EI|·cond_FP."""
    c = np.asarray(coefs, dtype=np.float64)
    P = mu.shape[0]
    with np.errstate(all="ignore"):
        muf, sf = c @ mu, np.sqrt((c * c) @ var)
        diff = muf - best
        z = diff / sf
        Phi, phi = O.normcdf(z), O.normpdf(z)
        T1, T2 = diff * Phi, sf * phi
        c_ei = (1 + z * z) * (np.abs(T1) + np.abs(T2)) + P * Phi * (np.abs(c[:, None] * mu).sum(0) + abs(best))
        ei = T1 + T2
        fp, tsum = np.ones(mu.shape[1]), np.zeros(mu.shape[1])
        for p in range(P):
            if y_max is None or (np.isinf(y_max[p]) and y_max[p] > 0):
                continue
            t = (y_max[p] - mu[p]) / np.sqrt(var[p])
            fp = fp * O.normcdf(t)
            tsum = tsum + np.where(np.isfinite(t), 1 + t * t, 0.0)
    return c_ei * fp + np.abs(ei) * fp * tsum
