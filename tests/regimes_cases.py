"""What tests/golden/make_regimes.py, tests/test_regimes_host.py, tests/test_gpu_regimes.py and tools/accuracy_regimes.py share: the
fixture's array encoding, the inputs of a case rebuilt from its stored parameters, the bars and the variance-clip rule.

The fixture holds, per model, a few datasets (X, y, candidates) and a list of cases (a dataset's name, the hyper-parameters,
cond(K) of the fp64 matrix, the 50-digit truths rounded to fp64, as full arrays).  tests/golden/regimes.json has everything but the
arrays, one case per line; the arrays lie one after the other in tests/golden/regimes_arrays.npy (float64; data_layout and
truth_layout give the order, "at" where a dataset's or a case's begin).  Together they stay below the 400 KB of gp_golden.json.

Bars, with u = 2⁻⁵³, rows = N or n(1+d), B = cond(K)·rows·u (the project's formula without its 1e-9 floor):
    logpdf  8·B·(1 + |ℓ|)        μ  8·B·(1 + max|μ|)        var  8·B·α² (Gibbs: max α(x)² over points and candidates)
    every gradient  100·B·(1 + max|want|)   — want: ∇μ, ∇σ², or the whole likelihood gradient of the model (Gibbs: ∂λ, ∂α, ∂σ stacked)
B >= rows·u >= 36u here; were B < 8u, the multiple of B is replaced by 64u (a sum of `rows` terms).

Variance clip: the device maps var ∈ (−1e-8, 0) to 0 and raises below; a candidate whose TRUE variance is <= 2·(var bar) + 1e-8 is
left out of the call (keep_mask) so that a rounding error cannot turn into another code path."""
import json
import os

import numpy as np

U = 2.0 ** -53
HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "regimes.json")            # header, datasets' sizes, the cases' parameters: one case per line
ARRAYS = os.path.join(HERE, "golden", "regimes_arrays.npy")   # every array, one flat float64 vector ("at": where an entry's begin)
KERNELS = ("matern32", "matern52", "sqexp")


def truth_layout(model, D):
    """[(key, shape)] of a case's truths in the order they are stored."""
    d, N = D["X"].shape
    M = D["Xs"].shape[1]
    if model == "plain":
        return [("logpdf", ()), ("mu", (M,)), ("var", (M,)), ("dmu", (d, M)), ("dvar", (d, M)), ("llgrad", (d + 2,))]
    if model == "grad":
        return [("logpdf", ()), ("mu", (M,)), ("var", (M,)), ("llgrad", (d + 3,))]
    return [("logpdf", ()), ("mu", (M,)), ("var", (M,)), ("dlam", (d, N)), ("damp", (N,)), ("dnoise", (N,))]


def data_layout(model, d, N, M):
    """[(key, shape)] of a dataset's arrays in the order they are stored."""
    return [("X", (d, N)), ("y", (N,))] + ([("dY", (d, N))] if model == "grad" else []) + [("Xs", (d, M))]


def _take(flat, at, layout, into):
    for k, shp in layout:
        n = int(np.prod(shp))
        into[k] = float(flat[at]) if shp == () else flat[at:at + n].reshape(shp).copy()
        at += n
    return at


def derived(model, D, c):
    """What a case's stored parameters imply: its name, the rows of its matrix, and the variance scale amp2 of the bars — α² as lifted
    (plain, gradient model), max α(x)² over points and candidates (Gibbs)."""
    d, N = D["X"].shape
    if model == "gibbs":
        name = f"{c['data']}-gm{c['gm']:g}-cl{c['clam']}-ca{c['camp']}-cs{c['csig']}"
        return dict(name=name, rows=N, amp2=float(max(gibbs_latents(D["X"], c)[1].max(), gibbs_latents(D["Xs"], c)[1].max()) ** 2))
    name = f"{c['data']}-{c['kernel']}-l{c['lam_rel']:g}-" + (f"a{c['amp']:g}-s{c['sig']:g}" if model == "plain" else f"s{c['sig']:g}-g{c['gsig']:g}")
    return dict(name=name, rows=N * (1 + d) if model == "grad" else N, amp2=(c["amp"] + 1e-8) ** 2)


_fx = None


def load():
    """The fixture with every dataset's arrays and every case's truths under their keys (read once per process)."""
    global _fx
    if _fx is None:
        with open(PATH) as f:
            fx = json.load(f)
        flat = np.load(ARRAYS)
        for model in ("plain", "grad", "gibbs"):
            for D in fx[model]["datasets"].values():
                _take(flat, D["at"], data_layout(model, D["d"], D["N"], D["M"]), D)
            for c in fx[model]["cases"]:
                D = fx[model]["datasets"][c["data"]]
                _take(flat, c["at"], truth_layout(model, D), c)
                c.update(derived(model, D, c))
        _fx = fx
    return _fx


# ------------------------------------------------------------------------------------------ inputs of a case
def prior_mean(X):
    return 1.0 + 0.1 * np.asarray(X).sum(0)


def plain_inputs(fx, c, shift=0.0):
    """X, y, Xs, lengthscale[d], amplitude, noise_std, mean_X, mean_Xs (None, None without a prior mean).  shift (here and below): added
    to every hyper-parameter / latent value — ∓1e-8 imitates the +1e-8 lift left out or applied twice."""
    D = fx["plain"]["datasets"][c["data"]]
    X, Xs = D["X"], D["Xs"]
    lam = np.full(X.shape[0], c["lam_rel"] * np.sqrt(X.shape[0]))
    return (X, D["y"], Xs, lam + shift, c["amp"] + shift, c["sig"] + shift, (prior_mean(X) if c["mean"] else None),
            (prior_mean(Xs) if c["mean"] else None))


def grad_inputs(fx, c, shift=0.0):
    """X, y, dY, Xs, lengthscale[d], amplitude, noise_std, grad_noise_std."""
    D = fx["grad"]["datasets"][c["data"]]
    X = D["X"]
    lam = np.full(X.shape[0], c["lam_rel"] * np.sqrt(X.shape[0]))
    return X, D["y"], D["dY"], D["Xs"], lam + shift, c["amp"] + shift, c["sig"] + shift, c["gsig"] + shift


GIBBS_AMP0, GIBBS_SIG0 = 0.3, 1e-2


def gibbs_latents(X, c):
    """λ(x) d×n, α(x) n, σ(x) n of a Gibbs case at the columns of X: log-linear fields,
        λ_l(x) = gm·C_λ^(x_l − ½),   α(x) = 0.3·C_α^((x_1+…+x_d)/d − ½),   σ(x) = 1e-2·C_σ^(x_1 − ½),
    so that over [0,1]^d the contrast max/min is C and the geometric mean the leading constant.  (α along the diagonal and at level
    0.3: the kernel's (α_i+α_j)/2 prefactor is not positive definite for every α(·); with this one 4 of the 72 cases fail the 50-digit
    Cholesky, with α along one axis or at level 1 more than the tenth the generator allows.)"""
    X = np.asarray(X, dtype=np.float64)
    lam = c["gm"] * float(c["clam"]) ** (X - 0.5)
    amp = GIBBS_AMP0 * float(c["camp"]) ** (X.mean(0) - 0.5)
    noi = GIBBS_SIG0 * float(c["csig"]) ** (X[0] - 0.5)
    return lam, amp, noi


def gibbs_inputs(fx, c, shift=0.0):
    """X, y, Xs, lam_X, amp_X, noise_X, lam_Xs, amp_Xs."""
    D = fx["gibbs"]["datasets"][c["data"]]
    lam, amp, noi = gibbs_latents(D["X"], c)
    lam_s, amp_s, _ = gibbs_latents(D["Xs"], c)
    return D["X"], D["y"], D["Xs"], lam + shift, amp + shift, noi + shift, lam_s + shift, amp_s + shift


# ------------------------------------------------------------------------------------------ the fp64 oracle on a case
def oracle_outputs(O, model, fx, c, shift=0.0):
    """The fp64 oracle's value of every truth of the case, as a dict with the truths' keys.  shift: added to every hyper-parameter
    (the Gibbs model: to every latent value) before the call — ∓1e-8 is the +1e-8 lift left out / applied twice."""
    if model == "plain":
        X, y, Xs, lam, amp, sig, mX, ms = plain_inputs(fx, c, shift)
        post = O.gp_fit(X, y, c["kernel"], lam, amp, sig, mean=mX)
        mu, var, dmu, dvar = O.gp_mean_and_var_grad(post, Xs, ms)
        _, g = O.gp_data_loglike_grad(X, y, c["kernel"], lam, amp, sig, mean=mX)
        return {"logpdf": post.logpdf, "mu": mu, "var": var, "dmu": dmu, "dvar": dvar, "llgrad": g}
    if model == "grad":
        X, y, dY, Xs, lam, amp, sig, gsig = grad_inputs(fx, c, shift)
        post = O.gradient_gp_fit(X, y, dY, c["kernel"], lam, amp, sig, gsig)
        mu, var, _, _ = O.gradient_gp_mean_and_var_grad(post, Xs)               # (the variance unclipped)
        _, g = O.gradient_gp_loglike_grad_allpairs(X, y, dY, c["kernel"], lam, amp, sig, gsig)
        return {"logpdf": post.logpdf, "mu": mu, "var": var, "llgrad": g}
    X, y, Xs, lam, amp, noi, lam_s, amp_s = gibbs_inputs(fx, c, shift)
    lp, dlam, damp, dnoise, _ = O.nonstationary_loglike_grad(X, y, lam, amp, noi)
    mu, var = O.nonstationary_mean_and_var(O.nonstationary_fit(X, y, lam, amp, noi), Xs, lam_s, amp_s, clip=False)
    return {"logpdf": lp, "mu": mu, "var": var, "llgrad": np.vstack([dlam, damp[None], dnoise[None]])}


def cond_of(O, model, fx, c):
    """cond(K) of the fp64 matrix the oracle factorises."""
    if model == "plain":
        X, _, _, lam, amp, sig, _, _ = plain_inputs(fx, c)
        h = O.finite_gp_params(c["kernel"], X.shape[0], lam, amp, sig)
        K = O.kernelmatrix(h, X) + h.noise_std ** 2 * np.eye(X.shape[1])
    elif model == "grad":
        X, _, _, _, lam, amp, sig, gsig = grad_inputs(fx, c)
        K = O.augmented_kernel_matrix(c["kernel"], X, lam, amp, sig, gsig)
    else:
        X, _, _, lam, amp, noi, _, _ = gibbs_inputs(fx, c)
        K = O.gibbs_kernel_matrix(X, lam, amp, X, lam, amp) + np.diag(noi ** 2)
    return float(np.linalg.cond(K))


# ------------------------------------------------------------------------------------------ bars
def unit(c):
    """B = cond(K)·rows·u of a case."""
    return c["cond"] * c["rows"] * U


def _mult(c, m):
    B = unit(c)
    return m * B if B >= 8 * U else 64 * U


def bar_logpdf(c, want):
    return _mult(c, 8) * (1 + abs(want))


def bar_var(c):
    return _mult(c, 8) * c["amp2"]          # (derived)


def bar_grad(c, want):
    return _mult(c, 100) * (1 + np.abs(want).max())


def keep_mask(c):
    """Candidates that stay in a prediction call (the variance-clip rule of the module docstring), from the fixture alone."""
    return np.asarray(c["var"]) > 2 * bar_var(c) + 1e-8


def gibbs_llgrad(c):
    """The Gibbs likelihood gradient as one array [(d+2), N]: ∂λ rows, ∂α, ∂σ."""
    return np.vstack([c["dlam"], c["damp"][None], c["dnoise"][None]])


def ratios(c, got, model, keep=None):
    """err/(B·scale) per quantity present in `got` (the unit in which the bars are 8 and 100), for reports and messages.  keep: the
    candidates `got` holds (the scales stay those of all candidates)."""
    out = {}
    B = unit(c)
    for k, v in got.items():
        want = gibbs_llgrad(c) if (model == "gibbs" and k == "llgrad") else np.asarray(c[k])
        scale = c["amp2"] if k == "var" else (1 + float(np.abs(want).max()))
        if keep is not None and k in ("mu", "var", "dmu", "dvar"):
            want = want[..., keep]
        err = float(np.abs(np.asarray(v) - want).max()) if want.size else 0.0
        out[k] = err / (B * scale)
    return out


LIMIT = {"logpdf": 8, "mu": 8, "var": 8, "dmu": 100, "dvar": 100, "llgrad": 100}


def check(c, got, model, what, frac=1.0, keep=None):
    """Asserts every quantity of `got` within frac × its bar of the case's truths; returns the ratios err/(B·scale)."""
    r = ratios(c, got, model, keep)
    B = unit(c)
    for k, v in r.items():
        lim = LIMIT[k] * (1.0 if B >= 8 * U else 64 * U / (LIMIT[k] * B)) * frac
        assert v <= lim, f"{what} {c['name']}: {k} err/B = {v:.3g} > {lim:.3g} (cond {c['cond']:.3g}, B {B:.3g})"
    return r


# ------------------------------------------------------------------------------------------ the device on a case
# Each returns [(what, got, keep)]: the outputs of one group of entry points as a dict with the truths' keys, and the candidates the
# prediction calls were given (keep_mask).  `g`: a handle on the case's dataset to reuse (updated in place), or None.  shift: see
# plain_inputs (the device is then given parameters that are off by that much).
def device_plain(api, fx, c, g=None, shift=0.0):
    X, y, Xs, lam, amp, sig, mX, ms = plain_inputs(fx, c, shift)
    keep = keep_mask(c)
    h = api.GP(X, y, c["kernel"]) if g is None else g
    try:
        first = {"logpdf": h.update(lam, amp, sig, mX)}
        ll, gr = h.loglike_grad()
        second = {"logpdf": ll, "llgrad": gr}
        third = {}
        if keep.any():
            Xk, mk = np.asfortranarray(Xs[:, keep]), (None if ms is None else ms[keep])
            first["mu"], first["var"] = h.predict(Xk, mk)
            third["mu"], third["var"], third["dmu"], third["dvar"] = h.predict_grad(Xk, mk)
    finally:
        if g is None:
            h.close()
    return [("update/predict", first, keep), ("loglike_grad", second, keep), ("predict_grad", third, keep)]


def device_grad(api, fx, c, g=None, shift=0.0):
    X, y, dY, Xs, lam, amp, sig, gsig = grad_inputs(fx, c, shift)
    keep = keep_mask(c)
    h = api.GradGP(X, y, dY, c["kernel"]) if g is None else g
    try:
        first = {"logpdf": h.update(lam, amp, sig, gsig)}
        ll, gr = h.loglike_grad()
        if keep.any():
            first["mu"], first["var"] = h.predict(np.asfortranarray(Xs[:, keep]))
    finally:
        if g is None:
            h.close()
    return [("update/predict", first, keep), ("loglike_grad", {"logpdf": ll, "llgrad": gr}, keep)]


def device_gibbs(api, fx, c, g=None, shift=0.0):
    X, y, Xs, lam, amp, noi, lam_s, amp_s = gibbs_inputs(fx, c, shift)
    keep = keep_mask(c)
    h = api.GibbsGP(X, y) if g is None else g
    try:
        first = {"logpdf": h.update(lam, amp, noi)}
        ll, dlam, damp, dnoise, _ = h.loglike_grad()
        if keep.any():
            first["mu"], first["var"] = h.predict(np.asfortranarray(Xs[:, keep]), np.asfortranarray(lam_s[:, keep]), amp_s[keep])
    finally:
        if g is None:
            h.close()
    return [("update/predict", first, keep), ("loglike_grad", {"logpdf": ll, "llgrad": np.vstack([dlam, damp[None], dnoise[None]])}, keep)]


DEVICE = {"plain": device_plain, "grad": device_grad, "gibbs": device_gibbs}
TAIL = 5


def device_append(api, model, fx, c, one_by_one):
    """A handle created and fitted on the first N − 5 points, the last 5 appended (in one block, or one by one), then logpdf and one
    prediction of the N-point posterior: (got, keep) with the truths' keys."""
    keep = keep_mask(c)
    steps = [(a, a + 1) for a in range(-TAIL, 0)] if one_by_one else [(-TAIL, None)]
    cut = lambda A, a, b: A[..., a:b] if b is not None and b != 0 else A[..., a:]          # noqa: E731
    if model == "plain":
        X, y, Xs, lam, amp, sig, mX, ms = plain_inputs(fx, c)
        h = api.GP(np.asfortranarray(X[:, :-TAIL]), y[:-TAIL], c["kernel"])
        try:
            h.update(lam, amp, sig, None if mX is None else mX[:-TAIL])
            for a, b in steps:
                lp = h.append(np.asfortranarray(cut(X, a, b)), cut(y, a, b), None if mX is None else cut(mX, a, b))
            got = {"logpdf": lp}
            if keep.any():
                got["mu"], got["var"] = h.predict(np.asfortranarray(Xs[:, keep]), None if ms is None else ms[keep])
        finally:
            h.close()
    elif model == "grad":
        X, y, dY, Xs, lam, amp, sig, gsig = grad_inputs(fx, c)
        h = api.GradGP(np.asfortranarray(X[:, :-TAIL]), y[:-TAIL], np.asfortranarray(dY[:, :-TAIL]), c["kernel"])
        try:
            h.update(lam, amp, sig, gsig)
            for a, b in steps:
                lp = h.append(np.asfortranarray(cut(X, a, b)), cut(y, a, b), np.asfortranarray(cut(dY, a, b)))
            got = {"logpdf": lp}
            if keep.any():
                got["mu"], got["var"] = h.predict(np.asfortranarray(Xs[:, keep]))
        finally:
            h.close()
    else:
        X, y, Xs, lam, amp, noi, lam_s, amp_s = gibbs_inputs(fx, c)
        h = api.GibbsGP(np.asfortranarray(X[:, :-TAIL]), y[:-TAIL])
        try:
            h.update(np.asfortranarray(lam[:, :-TAIL]), amp[:-TAIL], noi[:-TAIL])
            for a, b in steps:
                lp = h.append(np.asfortranarray(cut(X, a, b)), cut(y, a, b), np.asfortranarray(cut(lam, a, b)), cut(amp, a, b), cut(noi, a, b))
            got = {"logpdf": lp}
            if keep.any():
                got["mu"], got["var"] = h.predict(np.asfortranarray(Xs[:, keep]), np.asfortranarray(lam_s[:, keep]), amp_s[keep])
        finally:
            h.close()
    return got, keep


def is_corner(model, c):
    """The corner subset of the append tests: the extremes of λ and of the noise levels (every kernel, both sizes)."""
    if model == "plain":
        return c["data"] == "b" or (c["lam_rel"] in (0.01, 30.0) and c["amp"] == 1.2 and c["sig"] in (1e-3, 2.0))
    if model == "grad":
        return c["lam_rel"] in (0.05, 30.0)
    return c["gm"] in (0.05, 5.0) and c["clam"] in (1, 100)
