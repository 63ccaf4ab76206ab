"""Generates tests/golden/acq_tails.json: 50-digit truths (oracle/mp_oracle.acq_truth) of the EI × feasibility epilogue and its gradient
for exactly chosen fp64 moments, for tests/test_acq_tails_host.py and tests/test_gpu_acq_tails.py.  The encoding, the bars and the
oracle runners are those of tests/acq_tails_cases.py.  Run from the repository root (a few seconds, CPU only):

    python tests/golden/make_acq_tails.py

Groups (one device call each; every random draw from a generator seeded by the group's name)
  tail-s<σ>-b<b>   P = 1, coef 1: z = −37 … 8 in steps of 0.5 and −10^k, k = −8 … 0, for σf ∈ {1e-9, 1e-6, 1e-3, 0.3, 1, 50} × b ∈ {0, 1.7, −123.4};
                   μ = b + z·sqrt(σ²) as fp64 forms it, stored: the truth is of the stored μ.
  ei-p2, -p3, -p16 mixed-sign coefficients, z ∈ [−12, 6]; p2 and p3 hold four columns whose last variance is −1e-9 (clipped to 0).
  ei-p17, ei-p20   twins of ei-p16 (padded outputs of coefficient 0, y_max = +Inf).
  corners          σf = 0 with diff =, >, < 0, and the same behind a variance of −1e-9.
  fp-1, fp-2       feasibility only: t ∈ [−37, 8] for one finite constraint, two finite constraints (product >= 1e-280), the others +Inf.
  fp-neginf        y_max = −Inf: factor 0.
  eifp, eifp-tiny  EI × feasibility with the product >= 1e-280, and a small group below that (check = "tiny").
  s3-tail, s3-eifp the Bayesian-inference average over S = 3 samples.
  g-*              gradients (S = 1, d ∈ {1, 3}): the same regimes with ∇μ ~ N(0, 1), ∇σ² ~ σ²·N(0, 1), variance >= 1e-18, no y_max = −Inf.

Asserted before anything is written: the product groups' truths on their side of 1e-280; every twin's oracle result bitwise its
twin's.  The fp64 oracle's worst err/(u·cond), for values and for gradients, goes into the header: the device's bar is 4× that,
rounded up to a power of two (acq_tails_cases.device_C)."""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import gp_oracle as O  # noqa: E402
from oracle import mp_oracle as MP  # noqa: E402
import acq_tails_cases as A  # noqa: E402

INF = float("inf")
SIGMAS = (1e-9, 1e-6, 1e-3, 0.3, 1.0, 50.0)
BESTS = (0.0, 1.7, -123.4)


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def z_grid(step=0.5):
    z = list(np.arange(-37.0, 8.0 + 1e-9, step)) + [-(10.0 ** k) for k in range(-8, 1)]
    return np.array(sorted(set(float(t) for t in z)))


def group(name, kind, mu, var, coefs=None, y_max=None, best=None, dmu=None, dvar=None, check="bar"):
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if mu.ndim == 2:
        mu, var = mu[None], var[None]
    S, P, M = mu.shape
    g = dict(name=name, kind=kind, check=check, twin=None, P=P, S=S, M=M, d=0, mu=mu, var=var, best=best,
             coefs=None if coefs is None else np.asarray(coefs, dtype=np.float64), y_max=None if y_max is None else np.asarray(y_max, dtype=np.float64))
    if kind == "grad":
        g["dmu"], g["dvar"] = np.asarray(dmu, dtype=np.float64), np.asarray(dvar, dtype=np.float64)
        g["d"] = g["dmu"].shape[1]
        assert g["dmu"].shape == g["dvar"].shape == (P, g["d"], M) and var.min() >= 1e-18
    return g


def with_grads(name, d, mu, var, **kw):
    r = rng_of(name)
    P, M = np.shape(mu)
    return group(name, "grad", mu, var, dmu=r.standard_normal((P, d, M)), dvar=np.asarray(var)[:, None, :] * r.standard_normal((P, d, M)), **kw)


def ei_moments(name, P, M, zlo, zhi, best, clipped=0, coefs=None, cons=None):
    """Mixed-sign coefficients and P×M moments whose z runs over [zlo, zhi]; `clipped` columns in front of the middle one (z < 0 of order 1)
    carry −1e-9 as the last output's variance.  cons = (y_max, (tlo, thi)): outputs p > 0 with a finite constraint get t_p uniform in [tlo, thi]."""
    r = rng_of(name)
    c = r.uniform(0.3, 2.0, P) * np.where(np.arange(P) % 2 == 0, 1.0, -1.0)
    coefs = c if coefs is None else coefs
    var = r.uniform(0.05, 2.0, (P, M))
    if clipped:
        var[-1, M // 2 - clipped:M // 2] = -1e-9
    mu = r.standard_normal((P, M))
    if cons is not None:
        for p in range(1, P):
            if np.isfinite(cons[0][p]):
                var[p] = r.choice([1e-4, 0.25, 4.0], M)
                mu[p] = cons[0][p] - r.uniform(cons[1][0], cons[1][1], M) * np.sqrt(var[p])
    z = np.linspace(zlo, zhi, M)
    sf = np.sqrt((coefs * coefs) @ np.maximum(var, 0.0))
    mu[0] += (best + z * sf - coefs @ mu) / coefs[0]
    return coefs, mu, var


def fp_moments(name, ym, M, tlo, thi, floor_log10=None):
    """P×M moments with t_p = (ym_p − μ_p)/s_p uniform in [tlo_p, thi_p] for the finite constraints; redrawn until log10 of the product
    is above floor_log10."""
    from scipy.special import log_ndtr
    r = rng_of(name)
    P = len(ym)
    mu, var = r.standard_normal((P, M)), r.choice([1e-6, 0.09, 1.0, 2500.0], (P, M))
    for j in range(M):
        while True:
            t = np.array([r.uniform(tlo[p], thi[p]) for p in range(P)])
            fin = np.isfinite(ym)
            if floor_log10 is None or log_ndtr(t[fin]).sum() / np.log(10.0) > floor_log10:
                break
        for p in range(P):
            if np.isfinite(ym[p]):
                mu[p, j] = ym[p] - t[p] * np.sqrt(var[p, j])
    return mu, var


def build():
    G = []
    zt = z_grid()
    for sg in SIGMAS:
        for b in BESTS:
            var = np.full(zt.size, sg * sg)
            G.append(group(f"tail-s{sg:g}-b{b:g}", "value", [b + zt * np.sqrt(var)], [var], coefs=[1.0], best=b))
    for P, M, cl in ((2, 30, 4), (3, 30, 4), (16, 24, 0)):
        c, mu, var = ei_moments(f"ei-p{P}", P, M, -12.0, 6.0, 0.8, cl)
        G.append(group(f"ei-p{P}", "value", mu, var, coefs=c, best=0.8))
    G += [dict(name="ei-p17", twin="ei-p16", P=17), dict(name="ei-p20", twin="ei-p16", P=20)]
    G.append(group("corners", "value", [[1.5, 1.5, 2.5, 0.5, 2.5, 0.5]], [[0.0, -1e-9, 0.0, 0.0, -1e-9, -1e-9]], coefs=[1.0], best=1.5))
    tg = np.arange(-37.0, 8.0 + 1e-9, 0.5)
    s1 = np.array([1e-3, 0.3, 50.0])[np.arange(tg.size) % 3]
    G.append(group("fp-1", "value", [1.3 - tg * np.sqrt(s1 * s1), np.linspace(-1, 1, tg.size)], [s1 * s1, np.full(tg.size, 0.7)], y_max=[1.3, INF]))
    ym2 = np.array([0.7, INF, -2.0])
    mu, var = fp_moments("fp-2", ym2, 60, [-37, 0, -37], [8, 0, 8], -280.0)
    G.append(group("fp-2", "value", mu, var, y_max=ym2))
    mu, var = fp_moments("fp-neginf", np.array([0.0, 1.0]), 4, [-2, -2], [2, 2])
    G.append(group("fp-neginf", "value", mu, var, y_max=[-INF, 1.0]))

    def eifp(name, P, M, zr, tr, ym, check="bar", coefs=None):
        c, mu, var = ei_moments(name, P, M, zr[0], zr[1], 0.3, coefs=coefs, cons=(ym, tr))
        return group(name, "value", mu, var, coefs=c, y_max=ym, best=0.3, check=check)
    G.append(eifp("eifp", 2, 60, (-25.0, 6.0), (-20.0, 8.0), [INF, 0.4]))
    G.append(eifp("eifp-tiny", 2, 12, (-36.0, -30.0), (-30.0, -19.5), [INF, 0.4], check="tiny"))
    # S = 3
    r = rng_of("s3-tail")
    z3 = np.linspace(-37.0, 8.0, 60)
    sg3 = np.array([1e-3, 0.3, 1.0])
    G.append(group("s3-tail", "value", [[1.7 + (z3 + r.uniform(-0.4, 0.4, 60)) * np.sqrt(s * s)] for s in sg3],
                   [[np.full(60, s * s)] for s in sg3], coefs=[1.0], best=1.7))
    c3 = np.array([1.1, -0.6, 0.4])
    parts = [eifp(f"s3-eifp/{s}", 3, 20, (-20.0, 5.0), (-12.0, 6.0), [INF, 0.4, 1.0], coefs=c3) for s in range(3)]
    G.append(group("s3-eifp", "value", [p["mu"][0] for p in parts], [p["var"][0] for p in parts], coefs=c3,
                   y_max=[INF, 0.4, 1.0], best=0.3))
    # gradients
    z1 = np.arange(-37.0, 8.0 + 1e-9, 1.0)
    sg = np.repeat([1e-9, 1e-3, 1.0, 50.0], z1.size)
    zz = np.tile(z1, 4)
    G.append(with_grads("g-tail-d1", 1, [1.7 + zz * np.sqrt(sg * sg)], [sg * sg], coefs=[1.0], best=1.7))
    z15 = np.arange(-37.0, 8.0 + 1e-9, 1.5)
    sg = np.repeat([1e-6, 0.3], z15.size)
    zz = np.tile(z15, 2)
    G.append(with_grads("g-tail-d3", 3, [zz * np.sqrt(sg * sg)], [sg * sg], coefs=[1.0], best=0.0))
    for P, M, d in ((2, 20, 3), (3, 20, 1), (16, 12, 1)):
        c, mu, var = ei_moments(f"g-ei-p{P}", P, M, -12.0, 6.0, 0.8)
        G.append(with_grads(f"g-ei-p{P}", d, mu, var, coefs=c, best=0.8))
    G += [dict(name="g-ei-p17", twin="g-ei-p16", P=17), dict(name="g-ei-p20", twin="g-ei-p16", P=20)]
    t15 = np.arange(-37.0, 8.0 + 1e-9, 1.5)
    s1 = np.array([1e-3, 0.3, 50.0])[np.arange(t15.size) % 3]
    G.append(with_grads("g-fp-1", 1, [1.3 - t15 * np.sqrt(s1 * s1), np.linspace(-1, 1, t15.size)], [s1 * s1, np.full(t15.size, 0.7)], y_max=[1.3, INF]))
    mu, var = fp_moments("g-fp-2", ym2, 20, [-37, 0, -37], [8, 0, 8], -280.0)
    G.append(with_grads("g-fp-2", 3, mu, var, y_max=ym2))
    e = eifp("g-eifp", 3, 30, (-20.0, 5.0), (-12.0, 6.0), [INF, 0.4, 1.0])
    G.append(with_grads("g-eifp", 3, e["mu"][0], e["var"][0], coefs=e["coefs"], y_max=e["y_max"], best=0.3))
    return G


def fill_truths(g):
    M, d = g["M"], g["d"]
    g["truth"], g["cond"] = np.zeros(M), np.zeros(M)
    if g["kind"] == "grad":
        g["gtruth"], g["gcond"] = np.zeros((d, M)), np.zeros((d, M))
    for j in range(M):
        t = A.column_truth(MP, g, j)
        g["truth"][j], g["cond"][j] = t[0], t[1]
        if g["kind"] == "grad":
            g["gtruth"][:, j], g["gcond"][:, j] = t[2], t[3]


def main():
    G = build()
    by_name = {}
    for i, g in enumerate(G):
        if g.get("twin"):
            t = A.pad_outputs(by_name[g["twin"]], g["P"])
            t["name"], t["twin"] = g["name"], g["twin"]
            G[i] = g = t
        else:
            fill_truths(g)
        by_name[g["name"]] = g
    assert by_name["eifp"]["truth"].min() >= 1e-280 and by_name["fp-2"]["truth"].min() >= 1e-280, "a product group reaches below 1e-280"
    assert by_name["eifp-tiny"]["truth"].max() <= 1e-280, by_name["eifp-tiny"]["truth"]
    # the fp64 oracle's ratios
    worst = {"value": (0.0, None), "grad": (0.0, None)}
    per_group = {}
    for g in G:
        if g["check"] == "tiny":
            assert A.check_tiny(A.oracle_value(O, g))
            continue
        if g["kind"] == "value":
            rv, rg = A.ratio(A.oracle_value(O, g), g["truth"], g["cond"]), None
        else:
            acq, dacq = A.oracle_grad(O, g)
            rv, rg = A.ratio(acq, g["truth"], g["cond"]), A.ratio(dacq, g["gtruth"], g["gcond"])
        per_group[g["name"]] = [rv, rg]
        if rv > worst["value"][0]:
            worst["value"] = (rv, g["name"])
        if rg is not None and rg > worst["grad"][0]:
            worst["grad"] = (rg, g["name"])
        if g["twin"]:
            t = by_name[g["twin"]]
            a, b = (A.oracle_value(O, g), A.oracle_value(O, t)) if g["kind"] == "value" else (A.oracle_grad(O, g)[1], A.oracle_grad(O, t)[1])
            assert np.array_equal(a, b), f"{g['name']}: the padded outputs change the oracle's bits"
    for n, (rv, rg) in per_group.items():
        print(f"{n:18s} oracle err/(u·cond): value {rv:.3g}" + ("" if rg is None else f", gradient {rg:.3g}"))
    print("worst:", worst)
    assert np.isfinite(worst["value"][0]) and np.isfinite(worst["grad"][0])
    header = {"u": A.U, "dps": 50, "bars": "see tests/acq_tails_cases.py", "groups": len(G), "candidates": int(sum(g["M"] for g in G)),
              "oracle_ratio": {"value": worst["value"][0], "grad": worst["grad"][0]},
              "oracle_ratio_at": {"value": worst["value"][1], "grad": worst["grad"][1]},
              "device_C": {"value": A.device_C(worst["value"][0]), "grad": A.device_C(worst["grad"][0])}}
    lines = ['{"header":' + json.dumps(header, separators=(",", ":")) + ',"groups":[']
    enc = [json.dumps(A.encode_group(g), separators=(",", ":")) for g in G]
    lines += [ln + "," for ln in enc[:-1]] + [enc[-1] + "]}"]
    with open(A.PATH, "w") as f:
        f.write("\n".join(lines) + "\n")
    size = os.path.getsize(A.PATH)
    print("wrote", A.PATH, size, "bytes")
    assert size < A.SIZE_LIMIT, "the fixture must stay below the size the other fixtures keep to"


if __name__ == "__main__":
    main()
