"""Seeded battery over every acquisition and set-prediction entry point that goes through members_enqueue and the two epilogue
launchers (csrc/host_predict.inc): each call's returned arrays go into one .npz, so that two builds of the library can be compared
bit for bit.  The library is the one BOSS_LIB_PATH names (else the package's own):

    BOSS_LIB_PATH=/path/to/libbosship.so python tools/members_fold_dump.py --out a.npz
    python tools/members_fold_dump.py --compare a.npz b.npz        # numpy.array_equal on every array, exit status 1 on a difference

--no-set runs the same battery in a child process with BOSS_NO_SET_PREDICT=1 (the switch is read once per process) and writes
<out>.noset.npz beside the first file.

Shapes are the smallest that reach every branch: d = 3, M = 33 (one full and one partial tile of 32) and one M = 70, N = 130 and
N = 100 (the one-launch small kernel: no set gradient path), P in {1, 2}, S in {1, 3}; gradient-observation members with d = 2 and
50 points (150 rows); nonstationary members with host and with resident latents; a program-kernel handle with gradients; a member
list of unequal N; input-only, output-only and two-sided warps; the Monte-Carlo fitness calls; the moments-only calls.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, M0, S0 = 3, 33, 3
PS = [(1, 1), (2, 1), (1, 3), (2, 3)]


class Recorder:
    def __init__(self):
        self.out = {}

    def __call__(self, name, fn):
        """the arrays (and scalars) fn returns under name/0, name/1, ...; a refused call leaves its error code"""
        from boss_jl_amd import api
        assert f"{name}/0" not in self.out and f"{name}/err" not in self.out, name
        try:
            res = fn()
        except api.BossError as e:
            self.out[f"{name}/err"] = np.array([e.code])
            return None
        for i, a in enumerate(res if isinstance(res, tuple) else (res,)):
            if a is not None:
                self.out[f"{name}/{i}"] = np.array(a)
        return res


def plain_members(api, rng, N, kernel="matern52", d=D, S=S0):
    """gps[s][p] (P = 2) from one fit_batch per output, with per-sample prior means c_sp + g_sp'x; (gps, mean(s, p, Z), slopes)"""
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1] + 0.2 * np.cos(4 * X[-1])])
    c, gr = rng.uniform(-0.2, 0.2, (S, 2)), rng.uniform(-0.2, 0.2, (S, 2, d))
    mean = lambda s, p, Z: c[s, p] + gr[s, p] @ Z                                          # noqa: E731
    gps = [[None, None] for _ in range(S)]
    for p in range(2):
        lam, amp, sig = rng.uniform(0.35, 0.8, (d, S)), rng.uniform(0.8, 1.5, S), rng.uniform(0.04, 0.1, S)
        col, _, st = api.fit_batch(X, Y[p], kernel, lam, amp, sig, mean_X=np.stack([mean(s, p, X) for s in range(S)]))
        assert not st.any()
        for s in range(S):
            gps[s][p] = col[s]
    return gps, mean, gr, Y


def means_at(mean, gr, P, S, Z):
    M = Z.shape[1]
    ms = np.stack([np.stack([mean(s, p, Z) for p in range(P)]) for s in range(S)])
    mg = np.stack([np.stack([np.repeat(gr[s, p][:, None], M, axis=1) for p in range(P)]) for s in range(S)])
    return ms, mg


def fitness(api, P):
    """f(y) = y_0 + 0.1 y_{P-1}²"""
    op = api.FIT_OP
    return api.FitnessProgram(P, [0.1], [(op["SQUARE"], P - 1, -1), (op["MUL"], P + 1, P), (op["ADD"], 0, P + 2)], P + 3)


def warps(api, P, d=D):
    """input-only, output-only, both: x_k -> x_k + 0.1 sin x_k; (mu_p, sd_p) -> (2 mu_p + 0.5, 2 sd_p)"""
    op = api.FIT_OP
    ip = api.MeanProgram(d, 0, [([0.1], [(op["SIN"], k, -1), (op["MUL"], d + 1, d), (op["ADD"], k, d + 2)], d + 3) for k in range(d)])
    q = 2 * P
    outs = [([2.0, 0.5], [(op["MUL"], p, q), (op["ADD"], q + 2, q + 1)], q + 3) for p in range(P)]
    outs += [([2.0], [(op["MUL"], P + p, q)], q + 1) for p in range(P)]
    out_prog = api.MeanProgram(q, 0, outs)
    return {"in": api.WarpProgram(ip, P, None), "out": api.WarpProgram(None, P, out_prog), "both": api.WarpProgram(ip, P, out_prog)}


def sqexp_program(api, d=D):
    op = api.FIT_OP
    code, acc = [], None
    nid = 2 * d + 1                                               # inputs u, v, then the constant -0.5 at id 2d
    for k in range(d):
        code += [(op["SUB"], k, d + k), (op["SQUARE"], nid, -1)]
        sq, nid = nid + 1, nid + 2
        if acc is not None:
            code.append((op["ADD"], acc, sq))
            sq, nid = nid, nid + 1
        acc = sq
    code += [(op["MUL"], acc, 2 * d), (op["EXP"], nid, -1)]
    return api.KernelProgram(d, [-0.5], code, nid + 1)


def plain_battery(api, rec, rng, tag, gps, mean, gr, Y, M, full):
    """every plain-model row of the table at one member grid; full: all modes and the warps, else the core calls only"""
    Xs = np.asfortranarray(rng.uniform(-0.05, 1.05, (D, M)))
    mask = np.all((Xs >= 0) & (Xs <= 1), axis=0)
    cand = api.Candidates(Xs)
    best = float(Y[0].max()) - 0.3
    for P, S in PS:
        rows = [gps[s][:P] for s in range(S)]
        ms, mg = means_at(mean, gr, P, S, Xs)
        coefs, ymax = [1.0, 0.2][:P], [np.inf, 0.3][:P]
        t = f"{tag}/P{P}S{S}"
        modes = {"both": (ymax, best, mask), "best": (None, best, None)}
        if full:
            modes.update({"cons": (ymax, None, mask), "none": (None, None, None)})    # "none": par.mode == 0
        for mname, (ym, b, mk) in modes.items():
            for mm in ((False, True) if full or mname == "both" else (True,)):
                u = f"{t}/{mname}/{'mean' if mm else 'nomean'}"
                rec(f"{u}/acq_ei", lambda: api.acq_ei(rows, cand, coefs, ym, b, mk, ms if mm else None))
                if S == 1:
                    rec(f"{u}/acq_ei_grad", lambda: api.acq_ei_grad(rows[0], Xs, coefs, ym, b, mk, ms[0] if mm else None, mg[0] if mm else None))
                rec(f"{u}/acq_ei_grad_set", lambda: api.acq_ei_grad_set(rows, Xs, coefs, ym, b, mk, ms if mm else None, mg if mm else None))
        rec(f"{t}/argmax_only", lambda: api.acq_ei(rows, cand, coefs, ymax, best, mask, ms, want_acq=False)[1:])
        fit = fitness(api, P)
        eps = rng.standard_normal((P, S if S > 1 else 8))
        rec(f"{t}/mc", lambda: api.acq_ei_mc(rows, cand, fit, eps, ymax, best, mask, ms))
        rec(f"{t}/mc_grad", lambda: api.acq_ei_mc_grad(rows, Xs, fit, eps, ymax, best, mask, ms, mg))
        fit.close()
        if not full:
            continue
        for wname, w in warps(api, P).items():
            rec(f"{t}/warp_{wname}/predict", lambda: w.predict(rows, Xs, ms))
            rec(f"{t}/warp_{wname}/predict_grad", lambda: w.predict_grad(rows, Xs, ms, mg))
            rec(f"{t}/warp_{wname}/acq_ei", lambda: w.acq_ei(rows, Xs, coefs, ymax, best, mask, ms))
            rec(f"{t}/warp_{wname}/acq_ei_grad", lambda: w.acq_ei_grad(rows, Xs, coefs, ymax, best, mask, ms, mg))
            w.close()
    cand.close()


def moments_battery(api, rec, rng):
    d, M = D, M0
    for P, S in PS:
        mu, var = rng.standard_normal((S, P, M)), rng.uniform(0.01, 1.0, (S, P, M))
        dmu, dvar = rng.standard_normal((S, P, d, M)), rng.standard_normal((S, P, d, M))
        mask = rng.uniform(size=M) > 0.2
        coefs, ymax = [1.0, 0.2][:P], [np.inf, 0.3][:P]
        t = f"moments/P{P}S{S}"
        rec(f"{t}/acq_ei_moments", lambda: api.acq_ei_moments(mu, var, coefs, ymax, 0.3, mask))
        rec(f"{t}/acq_ei_moments_none", lambda: api.acq_ei_moments(mu, var, coefs))
        if S == 1:
            rec(f"{t}/acq_ei_grad_moments", lambda: api.acq_ei_grad_moments(mu[0], var[0], dmu[0], dvar[0], coefs, ymax, 0.3, mask))
        fit = fitness(api, P)
        eps = rng.standard_normal((P, S if S > 1 else 8))
        rec(f"{t}/mc_moments", lambda: api.acq_ei_mc_moments(mu, var, fit, eps, ymax, 0.3, mask))
        rec(f"{t}/mc_grad_moments", lambda: api.acq_ei_mc_grad_moments(mu, var, dmu, dvar, fit, eps, ymax, 0.3, mask))
        fit.close()


def grad_obs_battery(api, rec, rng):
    d, n, S, M = 2, 50, S0, M0                                   # n (1 + d) = 150 rows
    X = rng.uniform(0, 1, (d, n))
    w = rng.uniform(0.5, 2.0, d)
    y, dY = np.sin(X.T @ w), w[:, None] * np.cos(X.T @ w)[None, :]
    gps, _, st = api.ggp_fit_batch(X, y, dY, "matern52", rng.uniform(0.3, 1.5, (d, S)), rng.uniform(0.5, 2.0, S), rng.uniform(0.05, 0.3, S),
                                   rng.uniform(0.05, 0.3, S))
    assert not st.any()
    Xs = np.asfortranarray(rng.uniform(0.05, 0.95, (d, M)))
    cand = api.Candidates(Xs)
    best = float(y.max()) - 0.3
    rec("ggp/S3/acq_ei", lambda: api.acq_ei([[g] for g in gps], cand, [1.0], None, best))
    rec("ggp/S3/acq_ei_grad_set", lambda: api.acq_ei_grad_set([[g] for g in gps], Xs, [1.0], None, best))
    rec("ggp/S1/acq_ei_grad_set", lambda: api.acq_ei_grad_set([[gps[1]]], Xs, [1.0], None, best))
    rec("ggp/S1/acq_ei_grad", lambda: api.acq_ei_grad([gps[1]], Xs, [1.0], None, best))
    cand.close()
    for g in gps:
        g.close()


def ngp_battery(api, rec, rng):
    d, N, S, P, M = D, 130, S0, 2, M0
    X = rng.uniform(0, 1, (d, N))
    Y = np.stack([np.sin(3 * X).sum(0), X[0] - X[1]])
    lat_of = lambda Z, i: (0.5 + 0.2 * Z + 0.02 * i, 1.0 + 0.3 * Z[0] + 0.02 * i)         # noqa: E731  (λ d×·, α)
    gps = [[None] * P for _ in range(S)]
    for p in range(P):
        lam = np.stack([lat_of(X, p + P * s)[0] for s in range(S)], axis=2)
        amp = np.stack([lat_of(X, p + P * s)[1] for s in range(S)], axis=1)
        col, _, st = api.ngp_fit_batch(X, Y[p], lam, amp, np.full((N, S), 0.07), mean_X=np.stack([0.1 * s + 0.2 * X[1] for s in range(S)]))
        assert not st.any()
        for s in range(S):
            gps[s][p] = col[s]
    odd = api.GibbsGP(X[:, :70], Y[0][:70])                      # a member of another shape: the list goes member by member
    odd.update(lat_of(X[:, :70], 0)[0], lat_of(X[:, :70], 0)[1], np.full(70, 0.07))
    Xs = np.asfortranarray(rng.uniform(0.02, 0.98, (d, M)))
    mask = rng.uniform(size=M) > 0.2
    src = api.GP(X, 1.5 + 0.3 * np.sin(3 * X.sum(0)), "matern52")
    src.update([0.6, 0.7, 0.8], 1.3, 0.1)
    spec = ("lognormal", (-0.7, 0.5), "softplus", 0.1)
    for P_, S_ in PS:
        rows = [gps[s][:P_] for s in range(S_)]
        flat = [g for row in rows for g in row]
        n = len(flat)
        lam = np.stack([lat_of(Xs, i)[0] for i in range(n)], axis=2)
        amp = np.stack([lat_of(Xs, i)[1] for i in range(n)], axis=1)
        dl = np.zeros((d, d, M, n))
        for k in range(d):
            dl[k, k] = 0.2
        da = np.zeros((d, M, n))
        da[0] = 0.3
        ms = np.stack([0.1 * i + 0.2 * Xs[1] for i in range(n)])
        mg = np.zeros((n, d, M))
        mg[:, 1] = 0.2
        coefs, ymax = [1.0, 0.2][:P_], [np.inf, 0.3][:P_]
        t = f"ngp/P{P_}S{S_}"
        rec(f"{t}/predict_set", lambda: api.ngp_predict_set(flat, Xs, lam, amp, ms))
        rec(f"{t}/predict_set_nomean", lambda: api.ngp_predict_set(flat, Xs, lam, amp))
        rec(f"{t}/predict_grad_set", lambda: api.ngp_predict_grad_set(flat, Xs, lam, amp, dl, da, ms, mg))
        rec(f"{t}/predict_grad_set_nojac", lambda: api.ngp_predict_grad_set(flat, Xs, lam, amp))
        rec(f"{t}/acq_ei_grad_set", lambda: api.ngp_acq_ei_grad_set(rows, Xs, lam, amp, dl, da, coefs, ymax, 0.4, mask, ms, mg))
        rec(f"{t}/acq_ei_grad_set_nojac", lambda: api.ngp_acq_ei_grad_set(rows, Xs, lam, amp, None, None, coefs, None, 0.4))
        lats = [[api.NgpLatents([(src, spec), 0.6 + 0.01 * (p + P_ * s), 0.7], (src, spec)) for p in range(P_)] for s in range(S_)]
        flat_l = [L for row in lats for L in row]
        rec(f"{t}/predict_set_lat", lambda: api.ngp_predict_set_lat(flat, Xs, flat_l, ms))
        rec(f"{t}/predict_grad_set_lat", lambda: api.ngp_predict_grad_set_lat(flat, Xs, flat_l, ms, mg))
        rec(f"{t}/acq_ei_grad_set_lat", lambda: api.ngp_acq_ei_grad_set_lat(rows, Xs, lats, coefs, ymax, 0.4, mask, ms, mg))
        for L in flat_l:
            L.close()
    mixed = [gps[0][0], odd, gps[1][0]]
    lam = np.stack([lat_of(Xs, i)[0] for i in range(3)], axis=2)
    amp = np.stack([lat_of(Xs, i)[1] for i in range(3)], axis=1)
    rec("ngp/mixed/predict_set", lambda: api.ngp_predict_set(mixed, Xs, lam, amp))
    rec("ngp/mixed/predict_grad_set", lambda: api.ngp_predict_grad_set(mixed, Xs, lam, amp))
    rec("ngp/mixed/acq_ei_grad_set", lambda: api.ngp_acq_ei_grad_set([[g] for g in mixed], Xs, lam, amp, None, None, [1.0], None, 0.4))
    src.close(), odd.close()
    for row in gps:
        for g in row:
            g.close()


def special_members_battery(api, rec, rng):
    """a program-kernel handle with gradients (member by member), and a list of unequal N (member by member)"""
    d, N, M = D, 130, M0
    X = rng.uniform(0, 1, (d, N))
    y = np.sin(3 * X).sum(0)
    Xs = np.asfortranarray(rng.uniform(0.02, 0.98, (d, M)))
    cand = api.Candidates(Xs)
    prog = sqexp_program(api)
    ks = [api.KernelGP(X, y, prog, grad=True) for _ in range(S0)]
    for s, g in enumerate(ks):
        g.update([0.5 + 0.05 * s, 0.6, 0.7], 1.0, 0.05)
    best = float(y.max()) - 0.3
    rec("kprog/S3/acq_ei", lambda: api.acq_ei([[g] for g in ks], cand, [1.0], None, best))
    rec("kprog/S3/acq_ei_grad_set", lambda: api.acq_ei_grad_set([[g] for g in ks], Xs, [1.0], None, best))
    rec("kprog/S1/acq_ei_grad", lambda: api.acq_ei_grad([ks[0]], Xs, [1.0], None, best))
    for g in ks:
        g.close()
    prog.close()
    a, mean_a, gr_a, Y = plain_members(api, rng, 130, S=2)
    b, _, _, _ = plain_members(api, rng, 140, S=1)
    rows = [[a[0][0]], [b[0][0]], [a[1][0]]]
    rec("mixed/acq_ei", lambda: api.acq_ei(rows, cand, [1.0], None, best))
    rec("mixed/acq_ei_grad_set", lambda: api.acq_ei_grad_set(rows, Xs, [1.0], None, best))
    fit = fitness(api, 1)
    eps = rng.standard_normal((1, 3))
    rec("mixed/mc_grad", lambda: api.acq_ei_mc_grad(rows, Xs, fit, eps, None, best))
    w = warps(api, 1)["both"]
    rec("mixed/warp_acq_ei", lambda: w.acq_ei(rows, Xs, [1.0], None, best))
    rec("mixed/warp_acq_ei_grad", lambda: w.acq_ei_grad(rows, Xs, [1.0], None, best))
    w.close(), fit.close(), cand.close()
    for grid in (a, b):
        for row in grid:
            for g in row:
                g.close()


def battery():
    from boss_jl_amd import api
    api.load_library()
    rec = Recorder()
    rng = np.random.default_rng(20240607)
    for N, M, full in ((130, M0, True), (130, 70, False), (100, 9, False)):      # N = 100, 9 candidates: the one-launch small kernel
        gps, mean, gr, Y = plain_members(api, rng, N)
        plain_battery(api, rec, rng, f"plain/N{N}M{M}", gps, mean, gr, Y, M, full)
        for row in gps:
            for g in row:
                g.close()
    moments_battery(api, rec, rng)
    grad_obs_battery(api, rec, rng)
    ngp_battery(api, rec, rng)
    special_members_battery(api, rec, rng)
    rec.out["counters/set_launches"] = np.array(api._set_launches())
    rec.out["counters/set_grad_launches"] = np.array([api._set_grad_launches()])
    return rec.out


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    names = sorted(set(a.files) | set(b.files))
    bad = [k for k in names if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k], equal_nan=True)]
    errs = [k for k in a.files if k.endswith("/err")]
    print(f"{len(names)} arrays compared, {len(names) - len(bad)} equal, {len(bad)} differ; {len(errs)} refused calls in {a_path}")
    for k in bad[:40]:
        if k in a.files and k in b.files and a[k].shape == b[k].shape:
            print(f"  {k}: max |diff| {np.nanmax(np.abs(a[k].astype(float) - b[k].astype(float))):.3e}")
        else:
            print(f"  {k}: missing or of another shape")
    for k in errs:
        print(f"  refused: {k} code {a[k]}")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--no-set", action="store_true", help="also run the battery in a child process with BOSS_NO_SET_PREDICT=1")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    if not args.out:
        ap.error("--out or --compare is needed")
    out = battery()
    np.savez(args.out, **out)
    print(f"{len(out)} arrays -> {args.out}; set launches {out['counters/set_launches'].tolist()}, set gradient launches "
          f"{out['counters/set_grad_launches'].tolist()}", flush=True)
    if args.no_set:
        child = os.path.splitext(args.out)[0] + ".noset.npz"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", child], env=dict(os.environ, BOSS_NO_SET_PREDICT="1"), timeout=900)
        sys.exit(r.returncode)


if __name__ == "__main__":
    main()
