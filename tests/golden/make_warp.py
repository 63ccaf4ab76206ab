"""Generates tests/golden/warp.json: 50-digit truths of warped models for tests/test_warp_host.py and tests/test_gpu_warp.py.  Cases,
transforms and bars are those of tests/warp_cases.py.  Run from the repository root, on the CPU (about a minute):

    python tests/golden/make_warp.py

Per case: P plain GPs (oracle/mp_oracle.py's 50-digit Gram matrix, factor and kernel) fitted on the stored model-space data, evaluated
at the EXACT warped candidates w(x) — the warp itself runs at 50 digits.  Stored, rounded to fp64:
    X_, J                      w(x) and ∂x_/∂x (mp.diff)
    mu_, var_, dmu_, dvar_     model-space moments at w(x) and their gradients w.r.t. x_ (mp.diff of the wholes, as plain_truth takes them)
    mu, var, dmu, dvar         user space: out(mu_, sqrt(var_)), var = sd², gradients w.r.t. x by mp.diff of the WHOLE chain x -> result
    L                          max |∂(mu, var)/∂(mu_, var_)| at the truth (the bars' factor)
    fold_mu, .., fold_dvar     the moments stage at 50 digits on the ROUNDED (X_, J, mu_, var_, dmu_, dvar_): what the host twin is given
Asserted before anything is written: every nonzero Jacobian entry (of the input warp and of the output transform) lies in
[1e-3, 1e3]; the library's host twins meet the stage bounds (values 1e-13, gradients 1e-12, relative) and the chain's bars."""
import json
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import gp_oracle as O  # noqa: E402
from oracle import mp_oracle as MP  # noqa: E402
import warp_cases as W  # noqa: E402

KID = {"matern32": 0, "matern52": 1, "sqexp": 2}
mp.mp.dps = 50


def f64(a):
    return np.array(a, dtype=object).astype(np.float64)


def along(f, x, k):
    return lambda t: f(x[:k] + [t] + x[k + 1:])


def case_truth(name):
    du, dm, N, M, P, win, wout, kernel, _ = W.CASES[name]
    _, Xs, Xtr_, Y_ = W.data(name)
    lam, amp, sig = W.hyper(name)
    off = mp.mpf("1e-8")                                     # the +1e-8 lift of every hyper-parameter
    lam_m = [mp.mpf(float(v)) + off for v in lam]
    cols = MP._cols(Xtr_.tolist())
    gps = []
    conds = []
    for p in range(P):
        a_m, s_m = mp.mpf(float(amp[p])) + off, mp.mpf(float(sig[p])) + off
        delta = [mp.mpf(float(Y_[p, j])) - mp.mpf(W.PRIOR_MEAN) for j in range(N)]
        _, L, a = MP._logpdf_of(MP._plain_gram(KID[kernel], cols, lam_m, a_m, s_m), delta)
        gps.append((a_m, L, a))
        h = O.finite_gp_params(kernel, dm, lam, amp[p], sig[p])
        conds.append(float(np.linalg.cond(O.kernelmatrix(h, Xtr_) + h.noise_std ** 2 * np.eye(N))))

    def mu_at(p, x_):
        a_m, _, a = gps[p]
        return MP._dot([MP._k(KID[kernel], cols[i], x_, lam_m, a_m) for i in range(N)], a) + mp.mpf(W.PRIOR_MEAN)

    def var_at(p, x_):
        a_m, L, _ = gps[p]
        v = MP._fsub(L, [MP._k(KID[kernel], cols[i], x_, lam_m, a_m) for i in range(N)])
        return a_m * a_m - MP._dot(v, v) + mp.mpf("1e-18")

    def warp(x):
        return [mp.mpf(v) for v in win(x, mp)]

    def out(mus, sds):
        m, s = wout(mus, sds, mp)
        return list(m), list(s)

    def user(x):
        """(mu[P], var[P]) of the whole chain at the user-space point x."""
        x_ = warp(x)
        m, s = out([mu_at(p, x_) for p in range(P)], [mp.sqrt(var_at(p, x_)) for p in range(P)])
        return m, [v * v for v in s]

    def fold(mus, vars_, gmu, gvar, J):
        """The moments stage on given model-space arrays (lists of mpf): mu, var, dmu[P][du], dvar[P][du]."""
        sds = [mp.sqrt(v) for v in vars_]
        m, s = out(mus, sds)
        dmu_o, dvar_o = [], []
        for r in range(2 * P):
            pick = (lambda mm, ss, r=r: (out(mm, ss)[0] + out(mm, ss)[1])[r])
            a = [mp.diff(lambda t, q=q: pick(mus[:q] + [t] + mus[q + 1:], sds), mus[q]) for q in range(P)]
            b = [mp.diff(lambda t, q=q: pick(mus, sds[:q] + [t] + sds[q + 1:]), sds[q]) for q in range(P)]
            g_ = [sum(a[q] * gmu[q][kk] + b[q] * gvar[q][kk] / (2 * sds[q]) for q in range(P)) for kk in range(dm)]
            gx = [sum(J[kk][k] * g_[kk] for kk in range(dm)) for k in range(du)]
            if r < P:
                dmu_o.append(gx)
            else:
                dvar_o.append([2 * s[r - P] * v for v in gx])
        return m, [v * v for v in s], dmu_o, dvar_o

    c = {k: [] for k in ("X_", "J", "mu_", "var_", "dmu_", "dvar_", "mu", "var", "dmu", "dvar", "fold_mu", "fold_var", "fold_dmu", "fold_dvar")}
    Lmax = mp.mpf(0)
    pd_lo, pd_hi = mp.inf, mp.mpf(0)
    for j in range(M):
        x = [mp.mpf(float(v)) for v in Xs[:, j]]
        x_ = warp(x)
        J = [[mp.diff(along(lambda z, r=r: warp(z)[r], x, k), x[k]) for k in range(du)] for r in range(dm)]      # [r][k]
        mus = [mu_at(p, x_) for p in range(P)]
        vrs = [var_at(p, x_) for p in range(P)]
        gmu = [[mp.diff(along(lambda z, p=p: mu_at(p, z), x_, kk), x_[kk]) for kk in range(dm)] for p in range(P)]
        gvr = [[mp.diff(along(lambda z, p=p: var_at(p, z), x_, kk), x_[kk]) for kk in range(dm)] for p in range(P)]
        m, v = user(x)
        dm_u = [[mp.diff(along(lambda z, p=p: user(z)[0][p], x, k), x[k]) for k in range(du)] for p in range(P)]
        dv_u = [[mp.diff(along(lambda z, p=p: user(z)[1][p], x, k), x[k]) for k in range(du)] for p in range(P)]
        # ∂(mu, var)/∂(mu_, var_) at the truth
        G = lambda mm, vv: (lambda o: o[0] + [t * t for t in o[1]])(out(mm, [mp.sqrt(t) for t in vv]))          # noqa: E731
        for r in range(2 * P):
            for q in range(P):
                Lmax = max(Lmax, abs(mp.diff(lambda t: G(mus[:q] + [t] + mus[q + 1:], vrs)[r], mus[q])),
                           abs(mp.diff(lambda t: G(mus, vrs[:q] + [t] + vrs[q + 1:])[r], vrs[q])))
        # nonzero first derivatives of the transforms themselves: inside [1e-3, 1e3]
        sds = [mp.sqrt(t) for t in vrs]
        pds = [abs(e) for row in J for e in row]
        for r in range(2 * P):
            pick = (lambda mm, ss, r=r: (out(mm, ss)[0] + out(mm, ss)[1])[r])
            pds += [abs(mp.diff(lambda t, q=q: pick(mus[:q] + [t] + mus[q + 1:], sds), mus[q])) for q in range(P)]
            pds += [abs(mp.diff(lambda t, q=q: pick(mus, sds[:q] + [t] + sds[q + 1:]), sds[q])) for q in range(P)]
        nz = [e for e in pds if e > mp.mpf("1e-30")]
        pd_lo, pd_hi = min([pd_lo] + nz), max([pd_hi] + nz)
        # the stage on the rounded arrays
        r64 = lambda a: [[mp.mpf(float(e)) for e in row] for row in a]                                            # noqa: E731
        fm, fv, fdm, fdv = fold([mp.mpf(float(t)) for t in mus], [mp.mpf(float(t)) for t in vrs], r64(gmu), r64(gvr), r64(J))
        for key, val in (("X_", x_), ("J", J), ("mu_", mus), ("var_", vrs), ("dmu_", gmu), ("dvar_", gvr), ("mu", m), ("var", v), ("dmu", dm_u),
                         ("dvar", dv_u), ("fold_mu", fm), ("fold_var", fv), ("fold_dmu", fdm), ("fold_dvar", fdv)):
            c[key].append(f64(val))
    assert mp.mpf("1e-3") <= pd_lo and pd_hi <= mp.mpf("1e3"), (name, pd_lo, pd_hi)
    o = {"X_": np.stack(c["X_"], axis=1), "J": np.stack(c["J"]), "L": float(Lmax), "cond": conds, "amp": amp.tolist()}         # X_ dm×M, J [M][dm][du]
    for key in ("mu_", "var_", "mu", "var", "fold_mu", "fold_var"):
        o[key] = np.stack(c[key], axis=1)                                                                          # P×M
    for key in ("dmu_", "dvar_", "dmu", "dvar", "fold_dmu", "fold_dvar"):
        o[key] = np.stack(c[key], axis=2)                                                                          # P×d×M
    return o


def check_host_twin(B, name, c):
    """The library's host twins on the case: stage bounds and the chain's bars; returns the worst ratios."""
    du, dm, N, M, P = W.CASES[name][:5]
    _, Xs, _, _ = W.data(name)
    w = W.warp_program(B, name)
    X_, J = w.apply_host(Xs, True)
    rel = lambda got, want: float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))                   # noqa: E731
    nz = np.abs(c["J"]) > 0
    worst = {"X_": rel(X_, c["X_"]) / 1e-13, "J": rel(J[nz], c["J"][nz]) / 1e-12}
    assert np.all(J[~nz] == 0.0)
    mu, var, dmu, dvar = w.moments_host(c["mu_"], c["var_"], c["dmu_"], c["dvar_"], c["J"])
    worst.update(fold_mu=rel(mu, c["fold_mu"]) / 1e-13, fold_var=rel(var, c["fold_var"]) / 1e-13,
                 fold_dmu=rel(dmu, c["fold_dmu"]) / 1e-12, fold_dvar=rel(dvar, c["fold_dvar"]) / 1e-12)
    vb, gb = W.chain_bars(c, N)
    worst.update(chain_val=max(np.abs(mu - c["mu"]).max(), np.abs(var - c["var"]).max()) / vb,
                 chain_grad=max(np.abs(dmu - c["dmu"]).max(), np.abs(dvar - c["dvar"]).max()) / gb)
    assert all(v <= 1.0 for v in worst.values()), (name, worst)
    return worst


def main():
    import __graft_entry__ as entry
    entry.build()
    import boss_jl_amd as B
    cases, header = {}, {}
    for name in W.CASES:
        c = case_truth(name)
        header[name] = {k: float(f"{v:.3g}") for k, v in check_host_twin(B, name, c).items()}
        print(name, header[name], flush=True)
        cases[name] = {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    with open(W.PATH, "w") as f:
        json.dump({"dps": 50, "host_twin_worst_ratio": header, "cases": cases}, f)
        f.write("\n")
    print(f"wrote {W.PATH}: {os.path.getsize(W.PATH)} bytes")


if __name__ == "__main__":
    main()
