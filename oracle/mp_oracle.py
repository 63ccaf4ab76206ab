"""50-digit mpmath evaluation of the same GP formulas as gp_oracle.py (TEST INFRASTRUCTURE).

Independent of numpy/LAPACK rounding: used to pin the fp64 oracle (and, through it, the HIP path)
for small N.  Formulas: src/models/gradient_gp.jl:323-361,403 (explicit Cholesky algebra) and
src/models/gaussian_process.jl:216-248 (the +1e-8 parameter offsets, α²·κ(r/λ), σ²I noise).

`posterior` is the plain posterior of tests/golden/make_golden.py.  `plain_truth`, `grad_obs_truth` and `gibbs_truth` (second half
of the file) are the truths of tests/golden/make_regimes.py: candidate gradients, likelihood gradients, the gradient-observation
model and the Gibbs model, differentiated numerically at high precision.  `plain_cov_truth`, `grad_obs_pred_truth`, `gibbs_pred_truth`
and `kprog_truth` are the truths of tests/golden/make_regimes_more.py: posterior covariances, the candidate gradients of the
gradient-observation and Gibbs models, and program-kernel posteriors.  `acq_truth` (end of the file) is the truth of
tests/golden/make_acq_tails.py: the EI × feasibility acquisition of one candidate and its gradient, with the condition sums of the bars.
"""
from __future__ import annotations

import mpmath as mp

MATERN32, MATERN52, SQEXP = 0, 1, 2


def _kappa(kernel, r):
    if kernel == MATERN32:
        s = mp.sqrt(3) * r
        return (1 + s) * mp.e ** (-s)
    if kernel == MATERN52:
        s = mp.sqrt(5) * r
        return (1 + s + s * s / 3) * mp.e ** (-s)
    if kernel == SQEXP:
        return mp.e ** (-r * r / 2)
    raise ValueError(kernel)


def _k(kernel, xa, xb, lam, amp):
    r2 = mp.mpf(0)
    for k in range(len(lam)):
        t = (xa[k] - xb[k]) / lam[k]
        r2 += t * t
    return amp * amp * _kappa(kernel, mp.sqrt(r2))


def posterior(X, y, kernel, lengthscale, amplitude, noise_std, Xs, mean_X=None, mean_s=None,
              dps: int = 50):
    """Returns (logpdf, mu[M], var[M]) as python floats rounded from `dps`-digit arithmetic.
    X: d×N nested list/array, Xs: d×M.  var includes the +1e-18 prediction jitter, unclipped."""
    mp.mp.dps = dps
    d = len(X)
    N = len(X[0])
    M = len(Xs[0])
    off = mp.mpf("1e-8")
    lam = [mp.mpf(float(l)) + off for l in lengthscale]
    amp = mp.mpf(float(amplitude)) + off
    sig = mp.mpf(float(noise_std)) + off
    cols = [[mp.mpf(float(X[k][j])) for k in range(d)] for j in range(N)]
    scol = [[mp.mpf(float(Xs[k][j])) for k in range(d)] for j in range(M)]
    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(N):
            K[i, j] = _k(kernel, cols[i], cols[j], lam, amp)
        K[i, i] += sig * sig
    L = mp.cholesky(K)
    delta = mp.matrix([mp.mpf(float(y[j])) - (mp.mpf(float(mean_X[j])) if mean_X is not None else 0)
                       for j in range(N)])
    z = mp.lu_solve(L, delta)            # L is triangular; LU of it is itself
    a = mp.lu_solve(L.T, z)
    logdet = 2 * sum(mp.log(L[i, i]) for i in range(N))
    logpdf = -(N * mp.log(2 * mp.pi) + logdet + sum(z[i] * z[i] for i in range(N))) / 2
    mus, vars_ = [], []
    for j in range(M):
        ks = mp.matrix([_k(kernel, cols[i], scol[j], lam, amp) for i in range(N)])
        mu = sum(ks[i] * a[i] for i in range(N))
        if mean_s is not None:
            mu += mp.mpf(float(mean_s[j]))
        v = mp.lu_solve(L, ks)
        var = amp * amp - sum(v[i] * v[i] for i in range(N)) + mp.mpf("1e-18")
        mus.append(float(mu))
        vars_.append(float(var))
    return float(logpdf), mus, vars_


# ------------------------------------------------------------------------------------------------
# Truths for tests/golden/make_regimes.py.  Everything below is written from the models' defining
# formulas (Rasmussen & Williams 2006, eqs. 2.25-2.30 and 5.9 for the posterior and the marginal
# likelihood; Solak et al. 2003 for derivative observations; Gibbs 1997 / Paciorek & Schervish 2004
# for the nonstationary kernel) and differentiates NUMERICALLY at high precision (mp.diff, or a
# central difference of the whole likelihood) instead of restating the analytic κ', h, g, q profiles
# of gp_oracle.py: the two files share the kernels' definitions and nothing else.
# ------------------------------------------------------------------------------------------------
_OFF = "1e-8"


def _mpv(v):
    return [mp.mpf(float(t)) for t in v]


def _cols(X):
    d, N = len(X), len(X[0])
    return [[mp.mpf(float(X[k][j])) for k in range(d)] for j in range(N)]


def _fsub(L, b):
    """L z = b, L lower triangular (N² operations; mp.lu_solve would factor L again)."""
    n = len(b)
    z = [mp.mpf(0)] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s -= L[i, k] * z[k]
        z[i] = s / L[i, i]
    return z


def _bsub(L, z):
    """Lᵀ a = z."""
    n = len(z)
    a = [mp.mpf(0)] * n
    for i in range(n - 1, -1, -1):
        s = z[i]
        for k in range(i + 1, n):
            s -= L[k, i] * a[k]
        a[i] = s / L[i, i]
    return a


def _dot(a, b):
    return mp.fsum(x * y for x, y in zip(a, b))


def _logpdf_of(K, delta):
    """log N(delta; 0, K) and the pieces predictions reuse: (logpdf, L, a = K⁻¹delta).  Raises ZeroDivisionError/ValueError
    where K is not positive definite (mp.cholesky)."""
    n = len(delta)
    L = mp.cholesky(K)
    z = _fsub(L, delta)
    a = _bsub(L, z)
    logdet = 2 * mp.fsum(mp.log(L[i, i]) for i in range(n))
    return -(n * mp.log(2 * mp.pi) + logdet + _dot(z, z)) / 2, L, a


def _cdiff(f, theta, i, h):
    """Central difference of the scalar f along parameter i.  With dps digits, step h and conditioning c the result keeps about
    min(2·|log10 h|, dps − |log10 h| − log10 c) digits: callers choose dps and h so that both exceed 30."""
    tp, tm = list(theta), list(theta)
    tp[i] = theta[i] + h
    tm[i] = theta[i] - h
    return (f(tp) - f(tm)) / (2 * h)


def _plain_gram(kernel, cols, lam, amp, sig):
    n = len(cols)
    K = mp.matrix(n, n)
    for i in range(n):
        for j in range(i):
            K[i, j] = K[j, i] = _k(kernel, cols[i], cols[j], lam, amp)
        K[i, i] = amp * amp + sig * sig
    return K


def plain_truth(X, y, kernel, lengthscale, amplitude, noise_std, Xs, mean_X=None, mean_s=None, dps: int = 50,
                want_llgrad: bool = True, lift: str = _OFF):
    """Everything the plain model's tests compare: dict of python floats / nested lists rounded from `dps`-digit arithmetic.
        logpdf, mu[M], var[M] (with the 1e-18 jitter, unclipped), dmu[d][M], dvar[d][M]  (∂/∂x*, mp.diff of μ(x*) and σ²(x*) as wholes),
        llgrad[d+2] = ∂logpdf/∂(λ_1..λ_d, α, σ) AS GIVEN, i.e. through the +1e-8 lift (central difference of the whole likelihood at
        dps + 30 digits, h = 1e-25: ≥ 40 digits kept up to cond 1e15)."""
    mp.mp.dps = dps
    d, N, M = len(X), len(X[0]), len(Xs[0])
    off = mp.mpf(lift)
    cols, scol = _cols(X), _cols(Xs)
    delta = [mp.mpf(float(y[j])) - (mp.mpf(float(mean_X[j])) if mean_X is not None else 0) for j in range(N)]

    def ll(theta):
        lam = [t + off for t in theta[:d]]
        return _logpdf_of(_plain_gram(kernel, cols, lam, theta[d] + off, theta[d + 1] + off), delta)[0]

    theta = _mpv(lengthscale) + [mp.mpf(float(amplitude)), mp.mpf(float(noise_std))]
    lam, amp, sig = [t + off for t in theta[:d]], theta[d] + off, theta[d + 1] + off
    logpdf, L, a = _logpdf_of(_plain_gram(kernel, cols, lam, amp, sig), delta)
    out = {"logpdf": float(logpdf), "mu": [], "var": [], "dmu": [[0.0] * M for _ in range(d)], "dvar": [[0.0] * M for _ in range(d)]}

    def mu_at(xs):
        return _dot([_k(kernel, cols[i], xs, lam, amp) for i in range(N)], a)

    def var_at(xs):
        v = _fsub(L, [_k(kernel, cols[i], xs, lam, amp) for i in range(N)])
        return amp * amp - _dot(v, v) + mp.mpf("1e-18")

    for j in range(M):
        xs = scol[j]
        out["mu"].append(float(mu_at(xs) + (mp.mpf(float(mean_s[j])) if mean_s is not None else 0)))
        out["var"].append(float(var_at(xs)))
        for m in range(d):
            along = lambda f: (lambda t: f(xs[:m] + [t] + xs[m + 1:]))          # noqa: E731
            out["dmu"][m][j] = float(mp.diff(along(mu_at), xs[m]))
            out["dvar"][m][j] = float(mp.diff(along(var_at), xs[m]))
    if want_llgrad:
        mp.mp.dps = dps + 30
        h = mp.mpf("1e-25")
        out["llgrad"] = [float(_cdiff(ll, theta, i, h)) for i in range(d + 2)]
        mp.mp.dps = dps
    return out


# ---- gradient-observation model (Solak et al. 2003): cov(f(x), ∂f(x')/∂x'_l) = ∂k/∂x'_l, cov(∂f/∂x_l, ∂f/∂x'_m) = ∂²k/∂x_l∂x'_m ----
def _aug_gram(kernel, cols, lam, amp, sig, sgd):
    """The n(1+d) square matrix over [f(x_1..n), ∂f/∂x_1(x_1..n), …, ∂f/∂x_d(x_1..n)] with σ² on the value rows' diagonal and σ_∂² on the
    derivative rows'.  Every derivative block is a mixed partial of the scalar kernel by mp.diff with a multi-index over
    (x_1..x_d, x'_1..x'_d).  The training points must be pairwise distinct (Matérn-3/2 has no second derivative at r = 0, and the
    model's x_j + 1e-8 rule for near-coincident pairs is pinned elsewhere); a point against itself follows that rule, below."""
    n, d = len(cols), len(cols[0])
    Na = n * (1 + d)
    K = mp.matrix(Na, Na)

    def kk(*z):
        return _k(kernel, list(z[:d]), list(z[d:]), lam, amp)

    def idx(l, m):                  # multi-index: first derivative along x_l (l >= 0) and along x'_m (m >= 0)
        o = [0] * (2 * d)
        if l >= 0:
            o[l] += 1
        if m >= 0:
            o[d + m] += 1
        return tuple(o)

    # A point against itself: the model (gradient_gp.jl:143-159) takes the value at the point and every derivative block at
    # (x_i, x_i + 1e-8), the shifted point as fp64 forms it, and factorises the upper triangle mirrored.  The pair is then a pair of
    # distinct points like any other; only the value block and the mirroring differ.
    for i in range(n):
        K[i, i] = amp * amp + sig * sig
        z = tuple(cols[i]) + tuple(mp.mpf(float(t) + 1e-8) for t in cols[i])
        for l in range(d):
            K[i, n + l * n + i] = K[n + l * n + i, i] = mp.diff(kk, z, idx(-1, l))
            for m in range(l + 1):
                K[n + l * n + i, n + m * n + i] = K[n + m * n + i, n + l * n + i] = mp.diff(kk, z, idx(l, m))
            K[n + l * n + i, n + l * n + i] += sgd * sgd
    for i in range(n):
        for j in range(i):
            z = tuple(cols[i]) + tuple(cols[j])
            K[i, j] = K[j, i] = kk(*z)
            for l in range(d):
                v = mp.diff(kk, z, idx(-1, l))                  # cov(f(x_i), ∂f(x_j)/∂x_l)
                K[i, n + l * n + j] = K[n + l * n + j, i] = v
                K[j, n + l * n + i] = K[n + l * n + i, j] = -v  # k depends on x − x' only
                for m in range(l + 1):
                    w = mp.diff(kk, z, idx(l, m))               # cov(∂f(x_i)/∂x_l, ∂f(x_j)/∂x_m), symmetric in (l, m) and in (i, j)
                    for (p, q) in ((l, m), (m, l)):
                        K[n + p * n + i, n + q * n + j] = K[n + q * n + j, n + p * n + i] = w
                        K[n + p * n + j, n + q * n + i] = K[n + q * n + i, n + p * n + j] = w
    return K


def grad_obs_truth(X, y, dY, kernel, lengthscale, amplitude, noise_std, grad_noise_std, Xs, dps: int = 50,
                   want_llgrad: bool = True, lift: str = _OFF):
    """The gradient-observation model: logpdf of [y; dY rows], value μ[M] and var[M] (= α² − k*ᵀK⁻¹k*, no jitter, unclipped) at the
    candidates, llgrad[d+3] w.r.t. (λ, α, σ, σ_∂) as given (central difference of the whole likelihood, dps + 30 digits)."""
    mp.mp.dps = dps
    d, n, M = len(X), len(X[0]), len(Xs[0])
    off = mp.mpf(lift)
    cols, scol = _cols(X), _cols(Xs)
    yt = _mpv(y) + [mp.mpf(float(dY[l][j])) for l in range(d) for j in range(n)]

    def unpack(theta):
        return [t + off for t in theta[:d]], theta[d] + off, theta[d + 1] + off, theta[d + 2] + off

    def ll(theta):
        return _logpdf_of(_aug_gram(kernel, cols, *unpack(theta)), yt)[0]

    theta = _mpv(lengthscale) + [mp.mpf(float(amplitude)), mp.mpf(float(noise_std)), mp.mpf(float(grad_noise_std))]
    lam, amp, sig, sgd = unpack(theta)
    logpdf, L, a = _logpdf_of(_aug_gram(kernel, cols, lam, amp, sig, sgd), yt)
    out = {"logpdf": float(logpdf), "mu": [], "var": []}
    for c in range(M):
        xs = scol[c]
        ks = [_k(kernel, xs, cols[j], lam, amp) for j in range(n)]
        for l in range(d):
            for j in range(n):
                xj = cols[j]
                ks.append(mp.diff(lambda t: _k(kernel, xs, xj[:l] + [t] + xj[l + 1:], lam, amp), xj[l]))
        v = _fsub(L, ks)
        out["mu"].append(float(_dot(ks, a)))
        out["var"].append(float(amp * amp - _dot(v, v)))
    if want_llgrad:
        mp.mp.dps = dps + 30
        h = mp.mpf("1e-25")
        out["llgrad"] = [float(_cdiff(ll, theta, i, h)) for i in range(d + 3)]
        mp.mp.dps = dps
    return out


# ---- Gibbs / Paciorek-Schervish nonstationary kernel with per-point λ, α, σ ----
def _gibbs_factor(la, lb, dx):
    s = la * la + lb * lb
    return mp.sqrt(2 * la * lb / s) * mp.e ** (-dx * dx / s)


def _gibbs_k(xa, la, aa, xb, lb, ab):
    """((α(x)+α(y))/2)² Π_i sqrt(2 λ_i(x) λ_i(y) / (λ_i(x)² + λ_i(y)²)) exp(−(x_i − y_i)² / (λ_i(x)² + λ_i(y)²))."""
    k = ((aa + ab) / 2) ** 2
    for i in range(len(xa)):
        k *= _gibbs_factor(la[i], lb[i], xa[i] - xb[i])
    return k


def gibbs_truth(X, y, lam_X, amp_X, noise_X, Xs, lam_Xs, amp_Xs, mean_X=None, mean_s=None, dps: int = 50, want_llgrad: bool = True):
    """The nonstationary model with the latent values given at every point: logpdf, μ[M], var[M] (= α(x*)² − k*ᵀK⁻¹k* + 1e-18,
    unclipped) and, from ∂ℓ/∂θ = ½ tr((a aᵀ − K⁻¹) ∂K/∂θ) (R&W eq. 5.9) with ∂K_ij/∂λ_l(x_i) by mp.diff of the one factor that holds
    it, dlam[d][N], damp[N], dnoise[N], dmean[N].  Raises where K is not positive definite."""
    mp.mp.dps = dps
    d, N, M = len(X), len(X[0]), len(Xs[0])
    cols, scol = _cols(X), _cols(Xs)
    lam, lams = _cols(lam_X), _cols(lam_Xs)
    amp, amps, noi = _mpv(amp_X), _mpv(amp_Xs), _mpv(noise_X)
    delta = [mp.mpf(float(y[j])) - (mp.mpf(float(mean_X[j])) if mean_X is not None else 0) for j in range(N)]
    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(i):
            K[i, j] = K[j, i] = _gibbs_k(cols[i], lam[i], amp[i], cols[j], lam[j], amp[j])
        K[i, i] = amp[i] * amp[i] + noi[i] * noi[i]
    logpdf, L, a = _logpdf_of(K, delta)
    out = {"logpdf": float(logpdf), "mu": [], "var": []}
    for c in range(M):
        ks = [_gibbs_k(cols[i], lam[i], amp[i], scol[c], lams[c], amps[c]) for i in range(N)]
        v = _fsub(L, ks)
        out["mu"].append(float(_dot(ks, a) + (mp.mpf(float(mean_s[c])) if mean_s is not None else 0)))
        out["var"].append(float(amps[c] * amps[c] - _dot(v, v) + mp.mpf("1e-18")))
    if want_llgrad:
        Kinv = []                                                # rows of K⁻¹ (symmetric)
        for i in range(N):
            e = [mp.mpf(0)] * N
            e[i] = mp.mpf(1)
            z = _fsub(L, e)                                      # zero up to i: the generic solve, kept simple
            Kinv.append(_bsub(L, z))
        dlam = [[0.0] * N for _ in range(d)]
        damp, dnoise = [0.0] * N, [0.0] * N
        for i in range(N):
            G = [a[i] * a[j] - Kinv[i][j] for j in range(N)]
            sa = G[i] * amp[i]                                   # ½ G_ii ∂(α_i²)/∂α_i
            sl = [mp.mpf(0)] * d
            for j in range(N):
                if j == i:
                    continue
                sa += G[j] * K[i, j] * 2 / (amp[i] + amp[j])     # G_ij ∂K_ij/∂α_i = G_ij K_ij · 2/(α_i+α_j)  (each pair counted twice in the trace)
                for l in range(d):
                    dx, lb = cols[i][l] - cols[j][l], lam[j][l]
                    f = _gibbs_factor(lam[i][l], lb, dx)
                    df = mp.diff(lambda t: _gibbs_factor(t, lb, dx), lam[i][l])
                    sl[l] += G[j] * K[i, j] * df / f
            for l in range(d):
                dlam[l][i] = float(sl[l])
            damp[i] = float(sa)
            dnoise[i] = float(noi[i] * G[i])
        out.update(dlam=dlam, damp=damp, dnoise=dnoise, dmean=[float(t) for t in a])
    return out


# ------------------------------------------------------------------------------------------------
# Truths for tests/golden/make_regimes_more.py: posterior covariances of the three models, candidate gradients of the
# gradient-observation and the Gibbs model, and the posterior of a program kernel.  Same conventions as above (the +1e-8 lift, the
# 1e-18 jitter where the model has one, unclipped variances), and again no differentiation rule of a kernel: mp.diff of the scalar
# kernel by multi-index, mp.diff of μ and σ² as wholes, a central difference of the whole likelihood.
# ------------------------------------------------------------------------------------------------
def _cov_of(L, kstars, kss, jitter):
    """K** − VᵀV from the columns k*_c (lists) and the prior covariance kss(c, e); jitter on the diagonal.  M×M nested list of floats,
    mirrored from one triangle (exactly symmetric)."""
    M = len(kstars)
    V = [_fsub(L, ks) for ks in kstars]
    out = [[0.0] * M for _ in range(M)]
    for c in range(M):
        for e in range(c + 1):
            out[c][e] = out[e][c] = float(kss(c, e) - _dot(V[c], V[e]) + (jitter if c == e else 0))
    return out


def plain_cov_truth(X, kernel, lengthscale, amplitude, noise_std, Xs, dps: int = 50, lift: str = _OFF):
    """cov[M][M] of the plain model at the candidates: K** − K*ᵀ(K + σ²I)⁻¹K* + 1e-18·I, unclipped."""
    mp.mp.dps = dps
    off = mp.mpf(lift)
    cols, scol = _cols(X), _cols(Xs)
    lam, amp, sig = [t + off for t in _mpv(lengthscale)], mp.mpf(float(amplitude)) + off, mp.mpf(float(noise_std)) + off
    L = mp.cholesky(_plain_gram(kernel, cols, lam, amp, sig))
    kstars = [[_k(kernel, x, xs, lam, amp) for x in cols] for xs in scol]
    return _cov_of(L, kstars, lambda c, e: _k(kernel, scol[c], scol[e], lam, amp), mp.mpf("1e-18"))


def grad_obs_pred_truth(X, y, dY, kernel, lengthscale, amplitude, noise_std, grad_noise_std, Xs, dps: int = 50, lift: str = _OFF):
    """The gradient-observation model at the candidates: dmu[d][M] = (∂k*/∂x*_m)ᵀa, dvar[d][M] = −2(K⁻¹k*)ᵀ∂k*/∂x*_m (the prior
    variance α² is constant) and the value posterior's cov[M][M] = K** − k*ᵀK⁻¹k* (neither jittered nor clipped).  The rows of k* are
    those of grad_obs_truth; the rows of ∂k*/∂x*_m are mixed partials of the scalar kernel over (x*, x_j) by multi-index mp.diff, as
    _aug_gram forms its blocks."""
    mp.mp.dps = dps
    d, n, M = len(X), len(X[0]), len(Xs[0])
    off = mp.mpf(lift)
    cols, scol = _cols(X), _cols(Xs)
    yt = _mpv(y) + [mp.mpf(float(dY[l][j])) for l in range(d) for j in range(n)]
    lam = [t + off for t in _mpv(lengthscale)]
    amp, sig, sgd = (mp.mpf(float(t)) + off for t in (amplitude, noise_std, grad_noise_std))
    _, L, a = _logpdf_of(_aug_gram(kernel, cols, lam, amp, sig, sgd), yt)

    def kk(*z):
        return _k(kernel, list(z[:d]), list(z[d:]), lam, amp)

    def idx(m, l):                  # derivative along x*_m (m >= 0) and along (x_j)_l (l >= 0)
        o = [0] * (2 * d)
        if m >= 0:
            o[m] += 1
        if l >= 0:
            o[d + l] += 1
        return tuple(o)

    out = {"dmu": [[0.0] * M for _ in range(d)], "dvar": [[0.0] * M for _ in range(d)]}
    kstars = []
    for c in range(M):
        zs = [tuple(scol[c]) + tuple(cols[j]) for j in range(n)]
        ks = [kk(*z) for z in zs] + [mp.diff(kk, zs[j], idx(-1, l)) for l in range(d) for j in range(n)]
        kstars.append(ks)
        w = _bsub(L, _fsub(L, ks))                               # K⁻¹k*
        for m in range(d):
            dks = [mp.diff(kk, z, idx(m, -1)) for z in zs] + [mp.diff(kk, zs[j], idx(m, l)) for l in range(d) for j in range(n)]
            out["dmu"][m][c] = float(_dot(dks, a))
            out["dvar"][m][c] = float(-2 * _dot(dks, w))
    out["cov"] = _cov_of(L, kstars, lambda c, e: _k(kernel, scol[c], scol[e], lam, amp), 0)
    return out


def gibbs_pred_truth(X, y, lam_X, amp_X, noise_X, Xs, lam_Xs, amp_Xs, dlam_Xs, damp_Xs, mean_X=None, dps: int = 50):
    """The nonstationary model at the candidates: cov[M][M] (+1e-18 on the diagonal, unclipped) and dmu[d][M], dvar[d][M] with the
    candidate's latent values and Jacobians taken as given numbers (dlam_Xs[l][m][c] = ∂λ_l/∂x_m, damp_Xs[m][c] = ∂α/∂x_m): the
    derivative at t = 0 of μ (of σ²) along (x* + t·e_m, λ* + t·dlam[:, m], α* + t·damp[m]), by mp.diff of the whole expression."""
    mp.mp.dps = dps
    d, N, M = len(X), len(X[0]), len(Xs[0])
    cols, scol = _cols(X), _cols(Xs)
    lam, lams = _cols(lam_X), _cols(lam_Xs)
    amp, amps, noi = _mpv(amp_X), _mpv(amp_Xs), _mpv(noise_X)
    delta = [mp.mpf(float(y[j])) - (mp.mpf(float(mean_X[j])) if mean_X is not None else 0) for j in range(N)]
    K = mp.matrix(N, N)
    for i in range(N):
        for j in range(i):
            K[i, j] = K[j, i] = _gibbs_k(cols[i], lam[i], amp[i], cols[j], lam[j], amp[j])
        K[i, i] = amp[i] * amp[i] + noi[i] * noi[i]
    _, L, a = _logpdf_of(K, delta)
    kstars = [[_gibbs_k(cols[i], lam[i], amp[i], scol[c], lams[c], amps[c]) for i in range(N)] for c in range(M)]
    out = {"cov": _cov_of(L, kstars, lambda c, e: _gibbs_k(scol[c], lams[c], amps[c], scol[e], lams[e], amps[e]), mp.mpf("1e-18")),
           "dmu": [[0.0] * M for _ in range(d)], "dvar": [[0.0] * M for _ in range(d)]}
    for c in range(M):
        for m in range(d):
            dl = [mp.mpf(float(dlam_Xs[l][m][c])) for l in range(d)]
            da = mp.mpf(float(damp_Xs[m][c]))

            def kstar(t):
                xs = [scol[c][k] + (t if k == m else 0) for k in range(d)]
                ls = [lams[c][l] + t * dl[l] for l in range(d)]
                al = amps[c] + t * da
                return [_gibbs_k(cols[i], lam[i], amp[i], xs, ls, al) for i in range(N)], al

            def mu_t(t):
                return _dot(kstar(t)[0], a)

            def var_t(t):
                ks, al = kstar(t)
                v = _fsub(L, ks)
                return al * al - _dot(v, v) + mp.mpf("1e-18")

            out["dmu"][m][c] = float(mp.diff(mu_t, 0))
            out["dvar"][m][c] = float(mp.diff(var_t, 0))
    return out


def kprog_truth(f, X, y, lengthscale, amplitude, noise_std, Xs, mean_X=None, mean_s=None, no_grad_at=(), dps: int = 50,
                want_llgrad: bool = True, lift: str = _OFF):
    """The posterior under a program kernel k(x, y) = (α+1e-8)² f(x ⊘ (λ+1e-8), y ⊘ (λ+1e-8)); f(u, v) takes two lists of mpmath
    numbers (the caller wraps the 50-digit interpreter of the traced program).  Keys and conventions of plain_truth: logpdf, mu[M],
    var[M] (k(x*, x*) − k*ᵀK⁻¹k* + 1e-18, unclipped), dmu[d][M], dvar[d][M] (mp.diff of μ(x*) and σ²(x*) as wholes, the prior
    variance included; NaN at the candidates listed in no_grad_at, where f has a cusp), llgrad[d+2] (central difference of the whole
    likelihood).  Raises where K is not positive definite."""
    mp.mp.dps = dps
    d, N, M = len(X), len(X[0]), len(Xs[0])
    off = mp.mpf(lift)
    cols, scol = _cols(X), _cols(Xs)
    delta = [mp.mpf(float(y[j])) - (mp.mpf(float(mean_X[j])) if mean_X is not None else 0) for j in range(N)]

    def kf(xa, xb, lam, amp):
        return amp * amp * f([xa[k] / lam[k] for k in range(d)], [xb[k] / lam[k] for k in range(d)])

    def gram(lam, amp, sig):
        K = mp.matrix(N, N)
        for i in range(N):
            for j in range(i):
                K[i, j] = K[j, i] = kf(cols[i], cols[j], lam, amp)
            K[i, i] = kf(cols[i], cols[i], lam, amp) + sig * sig
        return K

    def ll(theta):
        return _logpdf_of(gram([t + off for t in theta[:d]], theta[d] + off, theta[d + 1] + off), delta)[0]

    theta = _mpv(lengthscale) + [mp.mpf(float(amplitude)), mp.mpf(float(noise_std))]
    lam, amp, sig = [t + off for t in theta[:d]], theta[d] + off, theta[d + 1] + off
    logpdf, L, a = _logpdf_of(gram(lam, amp, sig), delta)
    nan = float("nan")
    out = {"logpdf": float(logpdf), "mu": [], "var": [], "dmu": [[nan] * M for _ in range(d)], "dvar": [[nan] * M for _ in range(d)]}

    def mu_at(xs):
        return _dot([kf(cols[i], xs, lam, amp) for i in range(N)], a)

    def var_at(xs):
        v = _fsub(L, [kf(cols[i], xs, lam, amp) for i in range(N)])
        return kf(xs, xs, lam, amp) - _dot(v, v) + mp.mpf("1e-18")

    for j in range(M):
        xs = scol[j]
        out["mu"].append(float(mu_at(xs) + (mp.mpf(float(mean_s[j])) if mean_s is not None else 0)))
        out["var"].append(float(var_at(xs)))
        if j in no_grad_at:
            continue
        for m in range(d):
            along = lambda g: (lambda t: g(xs[:m] + [t] + xs[m + 1:]))          # noqa: E731
            out["dmu"][m][j] = float(mp.diff(along(mu_at), xs[m]))
            out["dvar"][m][j] = float(mp.diff(along(var_at), xs[m]))
    if want_llgrad:
        mp.mp.dps = dps + 30
        h = mp.mpf("1e-25")
        out["llgrad"] = [float(_cdiff(ll, theta, i, h)) for i in range(d + 2)]
        mp.mp.dps = dps
    return out


# ------------------------------------------------------------------------------------------------
# Truth of the acquisition epilogue for tests/golden/make_acq_tails.py: construct_ei's four variants
# (expected_improvement.jl:68-101,113-114) of ONE candidate and ONE hyper-parameter sample, from fp64 moments taken as exact.
# ------------------------------------------------------------------------------------------------
def _ncdf(z):
    """Φ(z) = erfc(−z/√2)/2: relative accuracy in both tails (mp.erfc), ±Inf included."""
    if mp.isinf(z):
        return mp.mpf(1) if z > 0 else mp.mpf(0)
    return mp.erfc(-z / mp.sqrt(2)) / 2


def _npdf(z):
    if mp.isinf(z):
        return mp.mpf(0)
    return mp.e ** (-z * z / 2) / mp.sqrt(2 * mp.pi)


def acq_truth(mu, var, coefs, y_max, best, dmu=None, dvar=None, dps: int = 50):
    """mu[P], var[P]: one candidate's moments; coefs[P] and best (None: no incumbent, expected_improvement.jl:68-73); y_max[P] or None
    (`constraints === nothing`; +Inf: the Infinity singleton, factor 1).  dmu / dvar: [P][d] moment gradients, or None.
    The variance is clipped as the device clips it: [−1e-8, 0) → 0; below −1e-8 the value is −Inf and the gradient 0.
    Returns python floats rounded from `dps`-digit arithmetic:
        value, cond                      the acquisition and its first-order condition sum (the bar of a result is C·u·cond):
                                         EI  (1+z²)(|T1|+|T2|) + P·Φ(z)(Σ|c_p μ_p| + |b|),  T1 = (μf − b)Φ(z), T2 = σf φ(z)
                                         FP  FP·Σ_p (1+t_p²)   (finite t_p only: a factor that is exactly 0 or 1 has no rounding)
                                         EI·FP  cond_EI·FP + |EI|·cond_FP
        grad[d], gcond[d]                the chain rule of ei_grad_point's comment and, term by term, the same construction: the sum
                                         of the absolute addends of Φ∇μf + φ∇σf times (1+z²)·P, of ∇FP times Σ_p(1+t_p²)·P, and the
                                         product rule over (EI, cond_EI, ∇EI, gcond_EI) × (FP, …)
        z, T1, T2, ei, fp, t[P]          the pieces (t_p: NaN for an output without a finite constraint)."""
    mp.mp.dps = dps
    P = len(mu)
    has_best, constrained = best is not None, y_max is not None
    d = 0 if dmu is None else len(dmu[0])
    out = {"value": 0.0, "cond": 0.0, "grad": [0.0] * d, "gcond": [0.0] * d, "z": float("nan"), "T1": 0.0, "T2": 0.0, "ei": float("nan"),
           "fp": float("nan"), "t": [float("nan")] * P}
    if not has_best and not constrained:
        return out
    m = _mpv(mu)
    v, live = [], []
    for p in range(P):
        x = float(var[p])
        if x < -1e-8:
            out["value"] = float("-inf")
            return out
        live.append(x > 0.0)
        v.append(mp.mpf(max(x, 0.0)))
    gm = [[mp.mpf(float(t)) for t in dmu[p]] for p in range(P)] if d else None
    gv = [[mp.mpf(float(t)) if live[p] else mp.mpf(0) for t in dvar[p]] for p in range(P)] if d else None
    zero = mp.mpf(0)
    ei, c_ei, dei, gc_ei = mp.mpf(1), zero, [zero] * d, [zero] * d
    if has_best:
        c = _mpv(coefs)
        b = mp.mpf(float(best))
        muf = mp.fsum(c[p] * m[p] for p in range(P))
        sf = mp.sqrt(mp.fsum(c[p] * c[p] * v[p] for p in range(P)))
        diff = muf - b
        if sf == 0:
            z = zero if diff == 0 else (mp.inf if diff > 0 else -mp.inf)
            Phi, phi = (zero if diff == 0 else _ncdf(z)), zero
            T1, T2, zz = (diff if diff > 0 else zero), zero, zero
        else:
            z = diff / sf
            Phi, phi = _ncdf(z), _npdf(z)
            T1, T2, zz = diff * Phi, sf * phi, z * z
        ei = T1 + T2
        c_ei = (1 + zz) * (abs(T1) + abs(T2)) + P * Phi * (mp.fsum(abs(c[p] * m[p]) for p in range(P)) + abs(b))
        for k in range(d):
            a1 = mp.fsum(c[p] * gm[p][k] for p in range(P))
            a2 = mp.fsum(c[p] * c[p] * gv[p][k] for p in range(P)) / (2 * sf) if sf != 0 else zero
            s1 = mp.fsum(abs(c[p] * gm[p][k]) for p in range(P))
            s2 = mp.fsum(abs(c[p] * c[p] * gv[p][k]) for p in range(P)) / (2 * sf) if sf != 0 else zero
            dei[k] = Phi * a1 + phi * a2
            gc_ei[k] = (1 + zz) * P * (Phi * s1 + phi * s2)
        out.update(z=float(z), T1=float(T1), T2=float(T2), ei=float(ei))
    fp, c_fp, dfp, gc_fp = mp.mpf(1), zero, [zero] * d, [zero] * d
    if constrained:
        ym = [mp.mpf(float(t)) for t in y_max]
        Phis, ts, tsum = [], [], zero
        for p in range(P):
            if mp.isinf(ym[p]) and ym[p] > 0:
                Phis.append(None)
                ts.append(None)
                continue
            s = mp.sqrt(v[p])
            if s == 0:
                t = mp.inf if ym[p] >= m[p] else -mp.inf
            else:
                t = (ym[p] - m[p]) / s
            Phis.append(_ncdf(t))
            ts.append(t)
            if not mp.isinf(t):
                tsum += 1 + t * t
                out["t"][p] = float(t)
        for q in Phis:
            if q is not None:
                fp *= q
        c_fp = fp * tsum
        for k in range(d):
            for p in range(P):
                if Phis[p] is None or not live[p] or mp.isinf(ts[p]):
                    continue
                others = mp.mpf(1)
                for q in range(P):
                    if q != p and Phis[q] is not None:
                        others *= Phis[q]
                s = mp.sqrt(v[p])
                b1, b2 = -gm[p][k] / s, -(ym[p] - m[p]) * gv[p][k] / (2 * s * v[p])
                w = others * _npdf(ts[p])
                dfp[k] += w * (b1 + b2)
                gc_fp[k] += tsum * P * w * (abs(b1) + abs(b2))
        out["fp"] = float(fp)
    if has_best and constrained:
        val, cond = ei * fp, c_ei * fp + abs(ei) * c_fp
        grad = [dei[k] * fp + ei * dfp[k] for k in range(d)]
        gcond = [gc_ei[k] * fp + abs(dei[k]) * c_fp + c_ei * abs(dfp[k]) + abs(ei) * gc_fp[k] for k in range(d)]
    elif has_best:
        val, cond, grad, gcond = ei, c_ei, dei, gc_ei
    else:
        val, cond, grad, gcond = fp, c_fp, dfp, gc_fp
    out.update(value=float(val), cond=float(cond), grad=[float(t) for t in grad], gcond=[float(t) for t in gcond])
    return out
