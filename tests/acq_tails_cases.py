"""What tests/golden/make_acq_tails.py, tests/test_acq_tails_host.py and tests/test_gpu_acq_tails.py share: the fixture's encoding, the
bars, the fp64 oracle (and its deliberately wrong variants) on a group, and the device on a group.

The fixture tests/golden/acq_tails.json holds groups of candidates for the EI × feasibility epilogue (csrc/acq_kernels.hpp), driven
through boss_acq_ei_moments / boss_acq_ei_grad_moments with exactly chosen fp64 moments.  A group is one device call: a header
(P, S, d, coefs, y_max, best) and M columns of moments with, per column, the 50-digit truth of oracle/mp_oracle.acq_truth rounded to
fp64 and the first-order condition sum `cond` it returns (4 significant digits).  Every float is a float.hex() string, so moments and
truths round-trip exactly; a row whose entries are all equal is {"c": value, "n": M}.  A group with "twin" holds nothing but a name
and P: its moments are its twin's, padded to P outputs of coefficient 0 and y_max = +Inf, and its truths are the twin's.

Bars, with u = 2⁻⁵³ (acq_truth's docstring has the formulas):  |got − truth| <= C·u·cond per candidate, for values and, per coordinate,
for gradients.  A Bayesian-inference average over S samples is a sum of S rounded terms scaled by a rounded 1/S:
    cond = mean_s cond_s + (S + 1)·mean_s |a_s|          (S − 1 additions and the scaling, each at most u·Σ|a_s|/S … u·Σ|a_s|).
Where the truth is not finite (a poisoned candidate: −Inf) the result must be that value.  C is not chosen here: the generator
measures the fp64 oracle's worst err/(u·cond) over the fixture, for values and for gradients, and writes both into the header;
the device's C is four times that, rounded up to a power of two (device_C).  check="tiny" groups (products below 1e-280, denormal or
zero) are asserted only to be finite, >= 0 and <= 1e-270."""
import json
import math
import os

import numpy as np

U = 2.0 ** -53
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "acq_tails.json")
SIZE_LIMIT = 400000
TINY_MAX = 1e-270
MUTANTS = ("phi_erf", "pdf_f32", "unclipped", "no_zero_branch", "neginf_skipped", "missing_half")


# ------------------------------------------------------------------------------------------ encoding
def enc(x):
    return float(x).hex()


def dec(s):
    return float.fromhex(s)


def enc_row(row):
    row = [float(t) for t in row]
    if len(row) > 1 and all(enc(t) == enc(row[0]) for t in row):
        return {"c": enc(row[0]), "n": len(row)}
    return [enc(t) for t in row]


def dec_row(r):
    if isinstance(r, dict):
        return np.full(r["n"], dec(r["c"]))
    return np.array([dec(t) for t in r], dtype=np.float64)


def enc_opt(v):
    return None if v is None else [enc(t) for t in np.asarray(v, dtype=np.float64).reshape(-1)]


def round_cond(x):
    """cond as the fixture stores it: 4 significant digits (it is part of the bar's definition, not a measured quantity)."""
    return float(f"{float(x):.3e}")


def encode_group(g):
    """A built group (numpy arrays, see build in make_acq_tails.py) as the JSON object of the fixture."""
    if g.get("twin"):
        return {"name": g["name"], "twin": g["twin"], "P": g["P"]}
    o = {"name": g["name"], "kind": g["kind"], "check": g["check"], "P": g["P"], "S": g["S"], "d": g["d"], "M": g["M"],
         "coefs": enc_opt(g["coefs"]), "y_max": enc_opt(g["y_max"]), "best": None if g["best"] is None else enc(g["best"]),
         "mu": [[enc_row(g["mu"][s, p]) for p in range(g["P"])] for s in range(g["S"])],
         "var": [[enc_row(g["var"][s, p]) for p in range(g["P"])] for s in range(g["S"])],
         "truth": enc_row(g["truth"]), "cond": [round_cond(t) for t in g["cond"]]}
    if g["kind"] == "grad":
        o["dmu"] = [[enc_row(g["dmu"][p, k]) for k in range(g["d"])] for p in range(g["P"])]
        o["dvar"] = [[enc_row(g["dvar"][p, k]) for k in range(g["d"])] for p in range(g["P"])]
        o["gtruth"] = [enc_row(g["gtruth"][k]) for k in range(g["d"])]
        o["gcond"] = [[round_cond(t) for t in g["gcond"][k]] for k in range(g["d"])]
    return o


PAD_MU, PAD_VAR = 0.25, 0.5          # moments of a twin's padded outputs (coefficient 0, y_max = +Inf: they change no bit)


def pad_outputs(g, P):
    """The group's header and moments padded to P outputs: copies, the original untouched."""
    k = P - g["P"]
    assert k > 0
    t = dict(g)
    t["P"] = P
    t["coefs"] = None if g["coefs"] is None else np.concatenate([g["coefs"], np.zeros(k)])
    t["y_max"] = None if g["y_max"] is None else np.concatenate([g["y_max"], np.full(k, np.inf)])
    S, _, M = g["mu"].shape
    t["mu"] = np.concatenate([g["mu"], np.full((S, k, M), PAD_MU) * (1 + np.arange(k))[None, :, None]], axis=1)
    t["var"] = np.concatenate([g["var"], np.full((S, k, M), PAD_VAR)], axis=1)
    if g["kind"] == "grad":
        t["dmu"] = np.concatenate([g["dmu"], np.full((k, g["d"], M), 0.75)], axis=0)
        t["dvar"] = np.concatenate([g["dvar"], np.full((k, g["d"], M), -0.125)], axis=0)
    return t


def decode_group(o):
    g = {k: o[k] for k in ("name", "kind", "check", "P", "S", "d", "M")}
    g["twin"] = None
    g["coefs"] = None if o["coefs"] is None else np.array([dec(t) for t in o["coefs"]])
    g["y_max"] = None if o["y_max"] is None else np.array([dec(t) for t in o["y_max"]])
    g["best"] = None if o["best"] is None else dec(o["best"])
    g["mu"] = np.array([[dec_row(r) for r in s] for s in o["mu"]])
    g["var"] = np.array([[dec_row(r) for r in s] for s in o["var"]])
    g["truth"] = dec_row(o["truth"])
    g["cond"] = np.array(o["cond"], dtype=np.float64)
    if g["kind"] == "grad":
        g["dmu"] = np.array([[dec_row(r) for r in p] for p in o["dmu"]])
        g["dvar"] = np.array([[dec_row(r) for r in p] for p in o["dvar"]])
        g["gtruth"] = np.array([dec_row(r) for r in o["gtruth"]])
        g["gcond"] = np.array(o["gcond"], dtype=np.float64)
    assert g["mu"].shape == g["var"].shape == (g["S"], g["P"], g["M"]) and g["truth"].shape == g["cond"].shape == (g["M"],), g["name"]
    return g


_fx = None


def load():
    """{"header": …, "groups": [group dicts with numpy arrays], "by_name": {…}} (read once per process)."""
    global _fx
    if _fx is None:
        with open(PATH) as f:
            raw = json.load(f)
        groups, by_name = [], {}
        for o in raw["groups"]:
            if o.get("twin"):
                g = pad_outputs(by_name[o["twin"]], o["P"])
                g["name"], g["twin"] = o["name"], o["twin"]
            else:
                g = decode_group(o)
            groups.append(g)
            by_name[g["name"]] = g
        _fx = {"header": raw["header"], "groups": groups, "by_name": by_name}
    return _fx


# ------------------------------------------------------------------------------------------ truths of a column (the generator; the regeneration test)
def column_truth(MP, g, j):
    """(truth, cond[, gtruth[d], gcond[d]]) of candidate j from oracle/mp_oracle.acq_truth, averaged over the group's samples as the
    module docstring says.  Values as stored: truth rounded once to fp64, cond to 4 digits."""
    import mpmath as mp
    S = g["S"]
    coefs = None if g["best"] is None else g["coefs"]
    outs = []
    for s in range(S):
        grad = g["kind"] == "grad"
        outs.append(MP.acq_truth(g["mu"][s, :, j], g["var"][s, :, j], coefs, g["y_max"], g["best"],
                                 g["dmu"][:, :, j] if grad else None, g["dvar"][:, :, j] if grad else None))
    vals = [o["value"] for o in outs]
    if S == 1:
        val, cond = vals[0], outs[0]["cond"]
    elif any(math.isinf(v) for v in vals):
        val, cond = float("-inf"), 0.0
    else:
        val = float(mp.fsum(mp.mpf(v) for v in vals) / S)
        cond = sum(o["cond"] for o in outs) / S + (S + 1) * sum(abs(v) for v in vals) / S
    res = (val, round_cond(cond))
    if g["kind"] == "grad":
        assert S == 1
        res += (outs[0]["grad"], [round_cond(t) for t in outs[0]["gcond"]])
    return res


# ------------------------------------------------------------------------------------------ bars
def device_C(ratio):
    """4 × the fp64 oracle's measured ratio, rounded up to a power of two."""
    return 2.0 ** math.ceil(math.log2(4.0 * ratio))


def errors(got, want):
    """|got − want| where want is finite; elsewhere 0 if got is that same value (NaN for NaN) and Inf if not."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(fin, err, np.where(same, 0.0, np.inf))


def misses(got, want, cond, C):
    """Boolean mask of the entries outside the bar C·u·cond (a NaN where a number is due is outside)."""
    return ~(errors(got, want) <= C * U * np.asarray(cond))


def ratio(got, want, cond):
    """Worst err/(u·cond) over the entries with cond > 0 (0.0 if there are none); an entry with cond = 0 must be exact and is
    judged by misses() alone."""
    err, cond = errors(got, want), np.asarray(cond, dtype=np.float64)
    pos = cond > 0
    if not pos.any():
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        r = err[pos] / (U * cond[pos])
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


def check_tiny(got):
    got = np.asarray(got)
    return bool(np.all(np.isfinite(got)) and np.all(got >= 0.0) and np.all(got <= TINY_MAX))


# ------------------------------------------------------------------------------------------ the fp64 oracle on a group
def _clip(var, mutant):
    """The device's variance rule on an array: [−1e-8, 0) → 0; (poisoned mask) below."""
    poison = np.any(var < -1e-8, axis=0)
    if mutant == "unclipped":
        return var, poison
    return np.where((var < 0) & (var >= -1e-8), 0.0, var), poison


class _patched:
    """The oracle module with one function swapped for a wrong one, restored on exit."""

    def __init__(self, O, mutant):
        self.O, self.mutant, self.saved = O, mutant, {}

    def __enter__(self):
        O = self.O
        if self.mutant == "phi_erf":
            from scipy.special import erf
            self.saved["normcdf"] = O.normcdf
            O.normcdf = lambda z: 0.5 * (1.0 + erf(np.asarray(z, dtype=np.float64) / math.sqrt(2.0)))
        elif self.mutant == "pdf_f32":
            self.saved["normpdf"] = O.normpdf
            orig = O.normpdf
            O.normpdf = lambda z: orig(np.asarray(z, dtype=np.float64).astype(np.float32).astype(np.float64))
        return self

    def __exit__(self, *a):
        for k, v in self.saved.items():
            setattr(self.O, k, v)


def _ei_lin(O, coefs, mu, var, best, mutant):
    if mutant != "no_zero_branch":
        return O.expected_improvement_lin(coefs, mu, var, best)
    c = np.asarray(coefs, dtype=np.float64)
    muf, sf = c @ mu, np.sqrt((c * c) @ var)
    diff = muf - best
    with np.errstate(divide="ignore", invalid="ignore"):
        z = diff / sf
        return diff * O.normcdf(z) + sf * O.normpdf(z)


def _feas(O, mu, var, y_max, mutant):
    if mutant == "neginf_skipped":
        y_max = np.where(np.isneginf(y_max), np.inf, y_max)
    return O.feas_prob(mu, var, y_max)


def oracle_value(O, g, mutant=None):
    """acq[M] of a group from gp_oracle.expected_improvement_lin / feas_prob, summed over the samples in ascending order and scaled
    by 1/S as the device does.  mutant: one of MUTANTS (the teeth of test_acq_tails_host.py)."""
    S, P, M = g["mu"].shape
    acc = np.zeros(M)
    with _patched(O, mutant), np.errstate(all="ignore"):
        for s in range(S):
            var, poison = _clip(g["var"][s], mutant)
            mu = g["mu"][s]
            if g["best"] is None and g["y_max"] is None:
                a, poison = np.zeros(M), np.zeros(M, bool)                 # expected_improvement.jl:68-70: the constant 0, moments unseen
            elif g["best"] is None:
                a = _feas(O, mu, var, g["y_max"], mutant)
            elif g["y_max"] is None:
                a = _ei_lin(O, g["coefs"], mu, var, g["best"], mutant)
            else:
                a = _ei_lin(O, g["coefs"], mu, var, g["best"], mutant) * _feas(O, mu, var, g["y_max"], mutant)
            acc = acc + np.where(poison, -np.inf, a)
    return acc * (1.0 / S) if S > 1 else acc


def oracle_grad(O, g, mutant=None):
    """(acq[M], dacq[d, M]) of a gradient group from gp_oracle.expected_improvement_lin_grad / feas_prob_grad (S = 1)."""
    assert g["S"] == 1
    mu, (var, poison) = g["mu"][0], _clip(g["var"][0], mutant)
    dmu, dvar = g["dmu"], np.where((var > 0)[:, None, :], g["dvar"], 0.0)
    d, M = g["d"], g["M"]
    with _patched(O, mutant), np.errstate(all="ignore"):
        if g["best"] is not None:
            ei, dei = O.expected_improvement_lin_grad(g["coefs"], mu, var, dmu, dvar * (2.0 if mutant == "missing_half" else 1.0), g["best"])
        if g["y_max"] is not None:
            fp, dfp = O.feas_prob_grad(mu, var, dmu, dvar, g["y_max"])
        if g["best"] is None and g["y_max"] is None:
            acq, dacq, poison = np.zeros(M), np.zeros((d, M)), np.zeros(M, bool)
        elif g["best"] is None:
            acq, dacq = fp, dfp
        elif g["y_max"] is None:
            acq, dacq = ei, dei
        else:
            acq, dacq = ei * fp, dei * fp + ei * dfp
    return np.where(poison, -np.inf, acq), np.where(poison[None, :], 0.0, dacq)


# ------------------------------------------------------------------------------------------ the device on a group
def device_value(api, g, var_scale=1.0, mask=None):
    """(acq[M], argmax, max) from boss_acq_ei_moments.  var_scale: every variance multiplied by it first (the device teeth)."""
    coefs = g["coefs"] if g["coefs"] is not None else np.zeros(g["P"])
    return api.acq_ei_moments(g["mu"], g["var"] * var_scale, coefs, g["y_max"], g["best"], mask)


def device_grad(api, g, var_scale=1.0, mask=None):
    """(acq[M], dacq[d, M]) from boss_acq_ei_grad_moments."""
    coefs = g["coefs"] if g["coefs"] is not None else np.zeros(g["P"])
    return api.acq_ei_grad_moments(g["mu"][0], g["var"][0] * var_scale, g["dmu"], g["dvar"] * var_scale, coefs, g["y_max"], g["best"], mask)


def ei_cond_fp64(O, mu, var, best, gm=None, gv=None):
    """cond (and gcond[d, M]) of acq_truth for P = 1, coef 1, EI only, evaluated in fp64: the bar between two device paths that were
    handed the same moments (test 6 of test_gpu_acq_tails.py), where no 50-digit truth is stored.  A bar needs one digit, not fifty."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    sf = np.sqrt(var)
    diff = mu - best
    z = diff / sf
    Phi, phi = O.normcdf(z), O.normpdf(z)
    cond = (1 + z * z) * (np.abs(diff * Phi) + sf * phi) + Phi * (np.abs(mu) + abs(best))
    if gm is None:
        return cond
    return cond, (1 + z * z)[None, :] * (Phi[None, :] * np.abs(gm) + phi[None, :] * np.abs(gv) / (2 * sf)[None, :])


def mean_cond(conds, vals):
    """The Bayesian-inference average's cond from the samples' (module docstring): arrays [S, M]."""
    S = len(conds)
    return np.mean(conds, axis=0) + (S + 1) * np.mean(np.abs(vals), axis=0)


def z_of(g):
    """z = (μf − b)/σf per candidate of a P = 1 EI group in fp64 (for the by-decade reports; not part of any bar)."""
    with np.errstate(all="ignore"):
        return (g["coefs"][0] * g["mu"][0, 0] - g["best"]) / (abs(g["coefs"][0]) * np.sqrt(np.maximum(g["var"][0, 0], 0.0)))


def decade(z):
    """Label of the |z| decade of a tail candidate: '-1e1..' for z <= −10, '-1e0..' for −10 < z <= −1, …, '+' for z > 0."""
    if not (z < 0):
        return "z>=0"
    return f"-1e{int(math.floor(math.log10(-z)))}"
