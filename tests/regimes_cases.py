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
left out of the call (keep_mask) so that a rounding error cannot turn into another code path.

The second half of the file holds the same for the second fixture, tests/golden/regimes_more.json (make_regimes_more.py,
test_regimes_more_host.py, test_gpu_regimes_more.py): further truths of the same cases and the program-kernel cases."""
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
        held = np.isfinite(want)                                   # (a truth left out on purpose is stored as NaN: regimes_more)
        scale = c["amp2"] if k in ("var", "cov") else (1 + float(np.abs(want[held]).max()))
        if keep is not None and k in ("mu", "var", "dmu", "dvar"):
            want, held = want[..., keep], held[..., keep]
        if keep is not None and k == "cov":
            want, held = want[np.ix_(keep, keep)], held[np.ix_(keep, keep)]
        err = float(np.asarray(np.abs(np.asarray(v) - want))[held].max()) if held.any() else 0.0
        out[k] = err / (B * scale)
    return out


LIMIT = {"logpdf": 8, "mu": 8, "var": 8, "dmu": 100, "dvar": 100, "llgrad": 100}


def check(c, got, model, what, frac=1.0, keep=None, limit=None):
    """Asserts every quantity of `got` within frac × its bar of the case's truths; returns the ratios err/(B·scale).  limit: the bars'
    multipliers per key where they are not LIMIT's (limit_more)."""
    mult = LIMIT if limit is None else limit
    r = ratios(c, got, model, keep)
    B = unit(c)
    for k, v in r.items():
        lim = mult[k] * (1.0 if B >= 8 * U else 64 * U / (mult[k] * B)) * frac
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


# ================================================================================================ the second fixture
# tests/golden/regimes_more.json + regimes_more_arrays.npy (tests/golden/make_regimes_more.py), for tests/test_regimes_more_host.py and
# tests/test_gpu_regimes_more.py: further truths of the cases above, referred to by name — cov[M][M] (all three models), dmu / dvar
# (gradient-observation and Gibbs model) — and the cases of a fourth model, "kprog": program-kernel posteriors on the plain datasets.
# Same encoding.  Bars: cov entries 8·B·amp2, every gradient 100·B·(1 + max|want|), kprog logpdf / mu / var as plain; the multiplier of
# a quantity whose fp64 oracle does not stay within an eighth of it is 8 × the oracle's worst ratio, rounded up to a power of two — the
# header holds the worst ratios and the multipliers (limit_more), chosen from the oracle alone.
PATH_MORE = os.path.join(HERE, "golden", "regimes_more.json")
ARRAYS_MORE = os.path.join(HERE, "golden", "regimes_more_arrays.npy")
MODELS_MORE = ("plain", "grad", "gibbs", "kprog")
KPROG_CLOSURES = ("expo", "ratquad", "persq", "dot1")          # of tests/kernel_program_cases.py
BASE_MULT = {"logpdf": 8, "mu": 8, "var": 8, "cov": 8, "dmu": 100, "dvar": 100, "llgrad": 100}


def more_layout(model, D):
    """[(key, shape)] of what the second fixture stores per case."""
    d = D["X"].shape[0]
    M = D["Xs"].shape[1]
    if model == "plain":
        return [("cov", (M, M))]
    if model in ("grad", "gibbs"):
        return [("dmu", (d, M)), ("dvar", (d, M)), ("cov", (M, M))]
    return [("logpdf", ()), ("mu", (M,)), ("var", (M,)), ("dmu", (d, M)), ("dvar", (d, M)), ("llgrad", (d + 2,))]


def gibbs_latent_jacobians(X, c):
    """(dlam d×d×n, damp d×n) of gibbs_latents at the columns of X, in closed form: ∂λ_l/∂x_m = δ_lm λ_l ln C_λ, ∂α/∂x_m = α ln C_α / d."""
    lam, amp, _ = gibbs_latents(X, c)
    d, n = lam.shape
    dlam = np.zeros((d, d, n))
    for l in range(d):
        dlam[l, l] = lam[l] * np.log(float(c["clam"]))
    return dlam, np.tile(amp * np.log(float(c["camp"])) / d, (d, 1))


def kprog_closure(c):
    import kernel_program_cases as cases
    return cases.CLOSURES[c["closure"]]


def kprog_derived(D, c):
    """name, rows and the variance scale amp2 = (α+1e-8)²·max_j f(u*_j, u*_j) of a kprog case (dot1 has no constant prior variance)."""
    import kernel_program_cases as cases
    d, N = D["X"].shape
    Us = D["Xs"] / (c["lam_rel"] * np.sqrt(d) + 1e-8)
    return dict(name=f"{c['data']}-{c['closure']}-l{c['lam_rel']:g}-a{c['amp']:g}-s{c['sig']:g}", rows=N,
                amp2=float((c["amp"] + 1e-8) ** 2 * cases.pairs(kprog_closure(c), Us, Us).max()))


def no_grad_at(c):
    """Candidates left out of a kprog case's dmu / dvar: the exponential kernel has a cusp at candidate 0, which lies on a training
    point (the device's convention there is pinned by tests/test_gpu_kernel_grad.py)."""
    return (0,) if c["closure"] == "expo" else ()


_fxm = None


def load_more():
    """{"header", model: [cases]}: every case of the first fixture that the second one names, as a copy with the further truths under
    their keys, and the kprog cases with theirs (read once per process)."""
    global _fxm
    if _fxm is None:
        fx = load()
        with open(PATH_MORE) as f:
            raw = json.load(f)
        flat = np.load(ARRAYS_MORE)
        out = {"header": raw["header"]}
        for model in ("plain", "grad", "gibbs"):
            by_name = {c["name"]: c for c in fx[model]["cases"]}
            out[model] = []
            for e in raw[model]:
                c = dict(by_name[e["case"]])
                _take(flat, e["at"], more_layout(model, fx[model]["datasets"][c["data"]]), c)
                out[model].append(c)
        out["kprog"] = []
        for c in raw["kprog"]:
            D = fx["plain"]["datasets"][c["data"]]
            _take(flat, c["at"], more_layout("kprog", D), c)
            c.update(kprog_derived(D, c))
            out["kprog"].append(c)
        _fxm = out
    return _fxm


def limit_more(fxm, model):
    """The multipliers of the second fixture's bars per key, from its header."""
    return dict(BASE_MULT, **fxm["header"]["multiplier"][model])


def multiplier_of(key, worst):
    """The rule by which make_regimes_more.py chooses a multiplier from the fp64 oracle's worst err/(B·scale)."""
    base = BASE_MULT[key]
    return base if worst <= base / 8 else int(2 ** np.ceil(np.log2(8 * worst)))


def kprog_programs(B):
    """{(closure name, d): api.KernelProgram traced with gradients} for the kprog cases; B is the imported package (library built)."""
    import kernel_program_cases as cases
    return {(n, d): B.DeviceKernel(cases.CLOSURES[n], d, grad=True).program for n in KPROG_CLOSURES for d in (2, 3)}


def mp_kernel(prog):
    """f(u, v) on two lists of mpmath numbers through the 50-digit program interpreter (fitness_mc_cases.mp_eval)."""
    from fitness_mc_cases import mp_eval
    return lambda u, v: mp_eval(prog, list(u) + list(v))[0]


# ------------------------------------------------------------------------------------------ the fp64 oracle on the further truths
def _pair_partials(prog, A, Bm):
    """(∂f/∂u, ∂f/∂v) of the program at every pair (A[:, i], Bm[:, j]): d×p×q each, by KernelProgram.grad."""
    d, p, q = A.shape[0], A.shape[1], Bm.shape[1]
    _, dU, dV = prog.grad(np.repeat(A, q, axis=1), np.tile(Bm, (1, p)))
    return dU.reshape(d, p, q), dV.reshape(d, p, q)


def kprog_oracle(prog, c, X, y, Xs, lam, amp, sig, mX, ms):
    """kernel_program_cases.Restated, and the formulas of kernel_grad_cases.RestatedGrad with the partials of the traced program
    (KernelProgram.grad) in place of closed forms: logpdf, mu, var (unclipped), dmu, dvar, llgrad; and cond(K)."""
    import scipy.linalg as sla
    import kernel_program_cases as cases
    ref = cases.Restated(kprog_closure(c), X, y, lam, amp, sig, Xs, None, mX, ms)
    N = X.shape[1]
    lamp = np.asarray(lam, float) + 1e-8
    G = np.outer(ref.a, ref.a) - sla.cho_solve((ref.L, True), np.eye(N), check_finite=False)
    Fu, Fv = _pair_partials(prog, ref.U, ref.U)
    dK = -ref.a2 * (Fu * ref.U[:, :, None] + Fv * ref.U[:, None, :]) / lamp[:, None, None]
    F = (ref.K - ref.s2 * np.eye(N)) / ref.a2
    llgrad = np.concatenate([0.5 * (G[None] * dK).sum((1, 2)), [0.5 * (G * F).sum() * 2.0 * (amp + 1e-8), 0.5 * np.trace(G) * 2.0 * (sig + 1e-8)]])
    Us = ref.scaled(Xs)
    W = sla.cho_solve((ref.L, True), ref.a2 * cases.gram(ref.f, ref.U, Us), check_finite=False)
    _, Fvs = _pair_partials(prog, ref.U, Us)
    _, su, sv = prog.grad(Us, Us)
    dmu = ref.a2 * np.einsum("i,dij->dj", ref.a, Fvs) / lamp[:, None]
    dvar = ref.a2 * ((su + sv) - 2.0 * np.einsum("ij,dij->dj", W, Fvs)) / lamp[:, None]
    return {"logpdf": ref.logpdf, "mu": ref.mu, "var": ref.var, "dmu": dmu, "dvar": dvar, "llgrad": llgrad}, ref.cond


def oracle_more(O, model, fx, c, shift=0.0, progs=None, jacobians=True):
    """[(got, keep)]: the fp64 oracle's value of every further truth of the case, with the candidates it was evaluated at (None: all;
    keep_mask where the oracle clips as the device does).  shift: see oracle_outputs.  jacobians=False: the Gibbs gradients with
    dlam_Xs = damp_Xs = None (the chain through the latent models left out)."""
    import scipy.linalg as sla
    if model == "plain":
        X, y, Xs, lam, amp, sig, mX, ms = plain_inputs(fx, c, shift)
        keep = keep_mask(c)
        if not keep.any():
            return []
        post = O.gp_fit(X, y, c["kernel"], lam, amp, sig, mean=mX)
        _, S = O.gp_mean_and_cov(post, Xs[:, keep], None if ms is None else ms[keep])
        return [({"cov": S}, keep)]
    if model == "grad":
        X, y, dY, Xs, lam, amp, sig, gsig = grad_inputs(fx, c, shift)
        post = O.gradient_gp_fit(X, y, dY, c["kernel"], lam, amp, sig, gsig)
        _, _, dmu, dvar = O.gradient_gp_mean_and_var_grad(post, Xs)
        Ks = O.augmented_cross_cov(c["kernel"], X, lam, amp, Xs)
        V = sla.solve_triangular(post.L, Ks, lower=True, check_finite=False)
        Kss = (amp + 1e-8) ** 2 * O.kappa(O.KERNEL_NAMES[c["kernel"]], O.scaled_distance(Xs, Xs, lam + 1e-8))
        return [({"dmu": dmu, "dvar": dvar, "cov": Kss - V.T @ V}, None)]
    if model == "gibbs":
        X, y, Xs, lam, amp, noi, lam_s, amp_s = gibbs_inputs(fx, c, shift)
        dlam_s, damp_s = gibbs_latent_jacobians(Xs, c) if jacobians else (None, None)
        post = O.nonstationary_fit(X, y, lam, amp, noi)
        _, _, dmu, dvar = O.nonstationary_mean_and_var_grad(post, Xs, lam_s, amp_s, dlam_s, damp_s)
        Ks = O.gibbs_kernel_matrix(X, lam, amp, Xs, lam_s, amp_s)
        V = sla.solve_triangular(post.L, Ks, lower=True, check_finite=False)
        S = O.gibbs_kernel_matrix(Xs, lam_s, amp_s, Xs, lam_s, amp_s) - V.T @ V + 1e-18 * np.eye(Xs.shape[1])
        return [({"dmu": dmu, "dvar": dvar, "cov": S}, None)]
    X, y, Xs, lam, amp, sig, mX, ms = plain_inputs(fx, c, shift)
    return [(kprog_oracle(progs[(c["closure"], X.shape[0])], c, X, y, Xs, lam, amp, sig, mX, ms)[0], None)]


# ------------------------------------------------------------------------------------------ the device on the further truths
# As DEVICE above: [(what, got, keep)], keep None where a call was given every candidate.  `g`: a handle on the case's dataset
# (kprog: and closure) to reuse, or None.
def device_plain_more(api, fx, c, g=None, shift=0.0, progs=None):
    X, y, Xs, lam, amp, sig, mX, ms = plain_inputs(fx, c, shift)
    keep = keep_mask(c)
    h = api.GP(X, y, c["kernel"]) if g is None else g
    out = []
    try:
        h.update(lam, amp, sig, mX)
        if keep.any():
            mu, S = h.predict_cov(np.asfortranarray(Xs[:, keep]), None if ms is None else ms[keep])
            assert np.array_equal(S, S.T), f"{c['name']}: predict_cov is not bitwise symmetric"
            out.append(("predict_cov", {"mu": mu, "cov": S, "var": np.diag(S).copy()}, keep))
    finally:
        if g is None:
            h.close()
    return out


def device_grad_more(api, fx, c, g=None, shift=0.0, progs=None):
    X, y, dY, Xs, lam, amp, sig, gsig = grad_inputs(fx, c, shift)
    keep = keep_mask(c)
    h = api.GradGP(X, y, dY, c["kernel"]) if g is None else g
    out = []
    try:
        h.update(lam, amp, sig, gsig)
        if keep.any():
            mu, var, dmu, dvar = h.predict_grad(np.asfortranarray(Xs[:, keep]))
            out.append(("predict_grad", {"mu": mu, "var": var, "dmu": dmu, "dvar": dvar}, keep))
        mu, S = h.predict_value_cov(Xs)
        out.append(("predict_value_cov", {"mu": mu, "cov": S}, None))
    finally:
        if g is None:
            h.close()
    return out


def device_gibbs_more(api, fx, c, g=None, shift=0.0, progs=None):
    X, y, Xs, lam, amp, noi, lam_s, amp_s = gibbs_inputs(fx, c, shift)
    dlam_s, damp_s = gibbs_latent_jacobians(Xs, c)
    keep = keep_mask(c)
    h = api.GibbsGP(X, y) if g is None else g
    out = []
    try:
        h.update(lam, amp, noi)
        if keep.any():
            Xk, lk, ak = np.asfortranarray(Xs[:, keep]), np.asfortranarray(lam_s[:, keep]), amp_s[keep]
            mu, var, dmu, dvar = h.predict_grad(Xk, lk, ak, dlam_s[:, :, keep], damp_s[:, keep])
            out.append(("predict_grad", {"mu": mu, "var": var, "dmu": dmu, "dvar": dvar}, keep))
            if c["clam"] == 1 and c["camp"] == 1:            # the Jacobians vanish: the call without them is the same derivative
                mu, var, dmu, dvar = h.predict_grad(Xk, lk, ak)
                out.append(("predict_grad without Jacobians", {"mu": mu, "var": var, "dmu": dmu, "dvar": dvar}, keep))
            mu, S = h.predict_cov(Xk, lk, ak)
            out.append(("predict_cov", {"mu": mu, "cov": S, "var": np.diag(S).copy()}, keep))
    finally:
        if g is None:
            h.close()
    return out


def device_kprog(api, fx, c, g=None, shift=0.0, progs=None):
    X, y, Xs, lam, amp, sig, mX, ms = plain_inputs(fx, c, shift)
    keep = keep_mask(c)
    h = api.KernelGP(X, y, progs[(c["closure"], X.shape[0])], grad=True) if g is None else g
    try:
        first = {"logpdf": h.update(lam, amp, sig, mX)}
        ll, gr = h.loglike_grad()
        third = {}
        if keep.any():
            Xk, mk = np.asfortranarray(Xs[:, keep]), (None if ms is None else ms[keep])
            first["mu"], first["var"] = h.predict(Xk, mk)
            third["mu"], third["var"], third["dmu"], third["dvar"] = h.predict_grad(Xk, mk)
    finally:
        if g is None:
            h.close()
    return [("update/predict", first, keep), ("loglike_grad", {"logpdf": ll, "llgrad": gr}, keep), ("predict_grad", third, keep)]


DEVICE_MORE = {"plain": device_plain_more, "grad": device_grad_more, "gibbs": device_gibbs_more, "kprog": device_kprog}
