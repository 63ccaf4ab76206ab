"""Randomized call sequences on the model handles (not part of the test suite by itself; tests/test_gpu_appended_large.py runs it):
the counterpart of tools/fuzz.py for api.GradGP and api.GibbsGP.  Per case a random sequence of 4 to 9 operations out of update /
predict (few-candidate, first-call and fused call sizes) / predict_grad / covariance / append (1, 1, 2, 5 or 33 points) / reserve /
loglike_grad / track / acq_ei_grad on one handle of about 128, 256, 1024 or 1280 rows (never above 1600), every result checked
against a fresh oracle fit of all points with tools/fuzz.py's rule tol = max(1e-9, cond(K) max(N, 2) 2^-53 16), gradient
quantities divided by 10.  No case is skipped or retried.

python tools/fuzz_models.py [n_cases] [seed] [grad|gibbs|both]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.linalg as sla
from boss_jl_amd import api
from oracle import gp_oracle as O

ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 12
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
which = sys.argv[3] if len(sys.argv) > 3 else "both"
KERN = ["matern32", "matern52", "sqexp"]
ROWS = [100, 127, 128, 129, 200, 250, 255, 256, 257, 300, 1016, 1023, 1024, 1025, 1100, 1270, 1279, 1280, 1281, 1400]
MS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 100, 224, 500]          # few-candidate, first-call and fused sizes of fuzz.py's MS
MAX_ROWS = 1600
OPS = ["predict", "predict", "predict", "grad", "cov", "append", "append", "append", "update", "reserve", "llgrad", "track", "acqgrad"]
t_start = time.time()


def cap256(rows):
    return -(-rows // 256) * 256


class Sequence:
    """What both models share: the operation loop, the track's life, the error/tolerance bookkeeping."""
    name = ""

    def __init__(self, case, rng):
        self.case, self.rng, self.ops, self.worst = case, rng, [], 0.0
        self.track = self.tcand = self.tXs = None
        self.tcap = 0

    def close_track(self):
        if self.track is not None:
            self.track.close()
            self.tcand.close()
            self.track = None

    def fail(self, what):
        print(f"CASE {self.case} {self.name} {self.describe()} ops={self.ops} append_path={api._append_path(self.g)}: {what}", flush=True)
        sys.exit(1)

    def note(self, e):
        self.worst = max(self.worst, e / self.tol)
        if not e <= self.tol:
            self.fail(f"error {e:.3e} > tol {self.tol:.1e}")

    def check_track(self):
        """moments of the track after every later operation.  A track holds the handle's storage at its creation + 256 rows, and
        that storage is at least the rows rounded up to 256: beyond that it may refuse (and is closed), within it must answer."""
        if self.track is None:
            return
        try:
            e = self.track_error()
        except api.BossError as ex:
            if "capacity" not in str(ex) or self.rows() <= self.tcap:
                raise
            self.close_track()
            return
        self.note(e)

    def run(self):
        for step in range(int(self.rng.integers(4, 10))):
            op = str(self.rng.choice(OPS))
            self.ops.append(op)
            try:
                e = getattr(self, "op_" + op)()
                if e is not None:
                    self.note(e)
                if op != "track":
                    self.check_track()
            except SystemExit:
                raise
            except Exception as ex:
                print(f"CASE {self.case} {self.name} {self.describe()} ops={self.ops} append_path={api._append_path(self.g)}: "
                      f"EXCEPTION {type(ex).__name__}: {ex}", flush=True)
                raise
        self.close_track()
        self.g.close()
        return self.worst

    def few_m(self, cap_pairs=None):
        M = int(self.rng.choice(MS))
        return M if cap_pairs is None else max(1, min(M, cap_pairs // self.npoints()))


class GradSequence(Sequence):
    name = "grad"

    def __init__(self, case, rng):
        super().__init__(case, rng)
        self.d = d = int(rng.choice([1, 2, 3, 8]))
        self.n = max(2, int(rng.choice(ROWS)) // (1 + d))
        self.kern = KERN[int(rng.integers(3))]
        self.X = rng.uniform(0, 1, (d, self.n))
        self.y, self.dY = self.obs(self.X)
        self.g = api.GradGP(self.X, self.y, self.dY, self.kern)
        self.cap = cap256(self.n * (1 + d))
        if rng.random() < 0.4:
            self.g.reserve(points=self.n + 9)
            self.cap = max(self.cap, cap256((self.n + 9) * (1 + d)))
        self.draw()
        self.fit(self.g.update(self.lam, *self.hyp))

    def obs(self, X):
        w = np.linspace(1.0, 2.0, self.d)[:, None]
        return np.sin(2 * np.pi * w * X).sum(0) / np.sqrt(self.d), 2 * np.pi * w * np.cos(2 * np.pi * w * X) / np.sqrt(self.d)

    def describe(self):
        return f"d={self.d} n={self.n} rows={self.rows()} {self.kern}"

    def rows(self):
        return self.n * (1 + self.d)

    def npoints(self):
        return self.n

    def draw(self):
        self.lam = self.rng.uniform(0.35, 0.7, self.d)
        self.hyp = (float(self.rng.uniform(0.8, 1.4)), float(self.rng.uniform(0.04, 0.1)), float(self.rng.uniform(0.08, 0.2)))

    def fit(self, lp):
        """the fresh oracle fit of all points, the tolerance from its conditioning, and the logpdf the device returned"""
        self.post = O.gradient_gp_fit(self.X, self.y, self.dY, self.kern, self.lam, *self.hyp)
        K = self.post.L @ self.post.L.T
        self.tol = max(1e-9, np.linalg.cond(K) * max(K.shape[0], 2) * 2.0 ** -53 * 16)
        assert self.g.n == self.n and self.g.N == self.rows(), (self.g.n, self.n)
        return abs(lp - self.post.logpdf) / (1 + abs(self.post.logpdf))

    def moments(self, Xs):
        Ks = O.augmented_cross_cov_allpairs(self.kern, self.X, self.lam, self.hyp[0], Xs)
        V = sla.solve_triangular(self.post.L, Ks, lower=True, check_finite=False)
        return Ks, V, Ks.T @ self.post.alpha, (self.hyp[0] + 1e-8) ** 2 - np.sum(V * V, axis=0)

    def cands(self, M):
        Xs = np.asfortranarray(self.rng.uniform(0, 1, (self.d, M)))
        if self.rng.random() < 0.3:
            Xs[:, 0] = self.X[:, int(self.rng.integers(self.n))]      # a candidate on a training point (head or appended)
        return Xs

    def op_predict(self):
        Xs = self.cands(self.few_m())
        mu, var = self.g.predict(Xs)
        _, _, mu_o, var_o = self.moments(Xs)
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(var - np.maximum(var_o, 0.0)).max() / self.hyp[0] ** 2)

    def op_grad(self):
        Xs = np.asfortranarray(self.rng.uniform(0, 1, (self.d, max(1, min(int(self.rng.choice([1, 3, 20, 65])), 6000 // self.n)))))
        mu, var, dmu, dvar = self.g.predict_grad(Xs)
        mu_o, var_o, dmu_o, dvar_o = O.gradient_gp_mean_and_var_grad(self.post, Xs)
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(dmu - dmu_o).max() / (1 + np.abs(dmu_o).max()),
                   np.abs(dvar - dvar_o).max() / (1 + np.abs(dvar_o).max())) / 10

    def op_cov(self):
        Xs = self.cands(int(self.rng.choice([1, 2, 7, 33, 70])))
        mu, S = self.g.predict_value_cov(Xs)
        _, V, mu_o, _ = self.moments(Xs)
        kid = O.KERNEL_NAMES[self.kern]
        S_o = (self.hyp[0] + 1e-8) ** 2 * O.kappa(kid, O.scaled_distance(Xs, Xs, self.lam + 1e-8)) - V.T @ V
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(S - S_o).max() / self.hyp[0] ** 2)

    def op_append(self):
        m = int(self.rng.choice([1, 1, 2, 5, 33]))
        while m > 1 and (self.n + m) * (1 + self.d) > MAX_ROWS:
            m = 1 if m <= 5 else 5
        if (self.n + m) * (1 + self.d) > MAX_ROWS:
            self.ops[-1] = "predict"
            return self.op_predict()
        Xn = self.rng.uniform(0, 1, (self.d, m))
        yn, dYn = self.obs(Xn)
        lp = self.g.append(Xn, yn, dYn)
        self.X, self.y, self.dY, self.n = np.hstack([self.X, Xn]), np.concatenate([self.y, yn]), np.hstack([self.dY, dYn]), self.n + m
        self.cap = max(self.cap, cap256(self.rows()))
        return self.fit(lp)

    def op_update(self):
        self.draw()
        e = self.fit(self.g.update(self.lam, *self.hyp))
        self.close_track()                                      # a track belongs to one set of hyper-parameters
        return e

    def op_reserve(self):
        """reserve leaves the handle unfitted: the update that must follow runs on the larger storage"""
        extra = int(self.rng.choice([1, 5, 40]))
        if (self.n + extra) * (1 + self.d) > MAX_ROWS + 256:
            extra = 1
        self.g.reserve(points=self.n + extra)
        self.cap = max(self.cap, cap256((self.n + extra) * (1 + self.d)))
        e = self.fit(self.g.update(self.lam, *self.hyp))
        self.close_track()
        return e

    def op_llgrad(self):
        ll, gr = self.g.loglike_grad()
        ll_o, gr_o = O.gradient_gp_loglike_grad_allpairs(self.X, self.y, self.dY, self.kern, self.lam, *self.hyp)
        return max(abs(ll - ll_o) / (1 + abs(ll_o)), np.abs(gr - gr_o).max() / (1 + np.abs(gr_o).max()) / 10)

    def op_track(self):
        if self.track is None:
            self.tXs = self.cands(int(self.rng.choice([1, 31, 64, 100])))
            self.tcand = api.Candidates(self.tXs)
            self.track = api.GradTrack(self.g, self.tcand)
            self.tcap = cap256(self.rows()) + 256
        self.check_track()

    def track_error(self):
        mu, var = self.track.moments()
        _, _, mu_o, var_o = self.moments(self.tXs)
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(var - var_o).max() / self.hyp[0] ** 2)

    def op_acqgrad(self):
        Xs = np.asfortranarray(self.rng.uniform(0, 1, (self.d, max(1, min(int(self.rng.choice([1, 3, 40])), 6000 // self.n)))))
        best = float(np.median(self.y))
        acq, dacq = api.acq_ei_grad([self.g], Xs, [1.0], None, best)
        mu_o, var_o, dmu_o, dvar_o = O.gradient_gp_mean_and_var_grad(self.post, Xs)
        vo = np.maximum(var_o, 0.0)
        want, dwant = O.expected_improvement_lin_grad([1.0], mu_o[None], vo[None], dmu_o[None], np.where(vo > 0, dvar_o, 0.0)[None], best)
        return max(np.abs(acq - want).max(), np.abs(dacq - dwant).max() / (1 + np.abs(dwant).max()) / 10)


class GibbsSequence(Sequence):
    name = "gibbs"

    def __init__(self, case, rng):
        super().__init__(case, rng)
        self.d = d = int(rng.choice([1, 2, 3, 8, 16]))
        self.N = int(rng.choice(ROWS))
        self.disc = None
        self.scale = np.ones(d)
        if d > 1 and rng.random() < 0.25:
            self.disc = np.zeros(d, bool)
            self.disc[1] = True
            self.scale[1] = 5.0
        self.use_mean = rng.random() < 0.5
        self.c = 1.0
        self.X = self.points(self.N)
        self.y = self.obs(self.X)
        self.g = api.GibbsGP(self.X, self.y, self.disc)
        self.cap = cap256(self.N)
        if rng.random() < 0.4:
            self.g.reserve(self.N + 40)
            self.cap = max(self.cap, cap256(self.N + 40))
        self.fit(self.g.update(*self.latents(self.X)))

    def points(self, M):
        return np.asfortranarray(self.rng.uniform(0, 1, (self.d, M)) * self.scale[:, None])

    def obs(self, X):
        return np.sin(2 * np.pi * X / self.scale[:, None]).sum(0) / np.sqrt(self.d) + 0.05 * self.rng.standard_normal(X.shape[1])

    def rnd(self, Z):
        return Z if self.disc is None else np.where(self.disc[:, None], np.rint(Z), Z)

    def latents(self, X, noise=True):
        """(λ, α[, σ], m) at X: the latent family of tests/test_gpu_ngp_append_track.py scaled by c, on the unit cube"""
        d, c = self.d, self.c
        Z = self.rnd(X) / self.scale[:, None]
        lam = c * (0.25 + 0.5 * Z ** 2 + (0.1 * np.arange(1, d + 1) / max(1.0, d / 3))[:, None]) * self.scale[:, None]
        amp = 1.0 + 0.4 * np.sin(3 * Z[0]) / c
        mean = 0.3 * X[0] if self.use_mean else None
        if not noise:
            return np.asfortranarray(lam), amp, mean
        return np.asfortranarray(lam), amp, 0.1 + 0.05 * (X[-1] / self.scale[-1]) ** 2, mean

    def describe(self):
        return f"d={self.d} N={self.N} disc={self.disc is not None} mean={self.use_mean}"

    def rows(self):
        return self.N

    def npoints(self):
        return self.N

    def fit(self, lp):
        lam, amp, noi, mean = self.latents(self.X)
        self.post = O.nonstationary_fit(self.X, self.y, lam, amp, noi, mean=mean, discrete=self.disc)
        K = self.post.L @ self.post.L.T
        self.tol = max(1e-9, np.linalg.cond(K) * max(self.N, 2) * 2.0 ** -53 * 16)
        self.amp2 = float(amp.max()) ** 2
        assert self.g.N == self.N, (self.g.N, self.N)
        return abs(lp - self.post.logpdf) / (1 + abs(self.post.logpdf))

    def op_predict(self):
        Xs = self.points(self.few_m())
        lam, amp, mean = self.latents(Xs, noise=False)
        mu, var = self.g.predict(Xs, lam, amp, mean)
        mu_o, var_o = O.nonstationary_mean_and_var(self.post, Xs, lam, amp, mean_s=mean)
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(var - var_o).max() / amp.max() ** 2)

    def grad_args(self, M):
        Xs = self.points(M)
        lam, amp, mean = self.latents(Xs, noise=False)
        mg = None
        if self.use_mean:
            mg = np.zeros((self.d, M))
            mg[0] = 0.3
        return Xs, lam, amp, mean, mg

    def op_grad(self):
        Xs, lam, amp, mean, mg = self.grad_args(int(self.rng.choice([1, 3, 20, 65, 224])))
        mu, var, dmu, dvar = self.g.predict_grad(Xs, lam, amp, None, None, mean, mg)
        mu_o, var_o, dmu_o, dvar_o = O.nonstationary_mean_and_var_grad(self.post, Xs, lam, amp, None, None, mean, mg)
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(dmu - dmu_o).max() / (1 + np.abs(dmu_o).max()),
                   np.abs(dvar - dvar_o).max() / (1 + np.abs(dvar_o).max())) / 10

    def op_cov(self):
        Xs = self.points(int(self.rng.choice([1, 2, 7, 33, 70])))
        lam, amp, mean = self.latents(Xs, noise=False)
        mu, S = self.g.predict_cov(Xs, lam, amp, mean)
        Xsr = self.rnd(Xs)
        Ks = O.gibbs_kernel_matrix(self.rnd(self.X), self.post.lam_X, self.post.amp_X, Xsr, lam, amp)
        V = sla.solve_triangular(self.post.L, Ks, lower=True, check_finite=False)
        S_o = O.gibbs_kernel_matrix(Xsr, lam, amp, Xsr, lam, amp) - V.T @ V + 1e-18 * np.eye(Xs.shape[1])
        S_o[np.diag_indices(Xs.shape[1])] = O.clip_var(np.diag(S_o))
        mu_o, _ = O.nonstationary_mean_and_var(self.post, Xs, lam, amp, mean_s=mean, clip=False)
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(S - S_o).max() / amp.max() ** 2)

    def op_append(self):
        n = int(self.rng.choice([1, 1, 2, 5, 33]))
        if self.N + n > MAX_ROWS:
            n = 1
        if self.N + n > MAX_ROWS:
            self.ops[-1] = "predict"
            return self.op_predict()
        Xn = self.points(n)
        yn = self.obs(Xn)
        lp = self.g.append(Xn, yn, *self.latents(Xn))
        self.X, self.y, self.N = np.asfortranarray(np.hstack([self.X, Xn])), np.concatenate([self.y, yn]), self.N + n
        self.cap = max(self.cap, cap256(self.N))
        return self.fit(lp)

    def op_update(self):
        self.c = float(self.rng.uniform(0.9, 1.3))
        e = self.fit(self.g.update(*self.latents(self.X)))
        self.close_track()
        return e

    def op_reserve(self):
        extra = int(self.rng.choice([1, 40, 200]))
        self.g.reserve(self.N + extra)
        self.cap = max(self.cap, cap256(self.N + extra))
        e = self.fit(self.g.update(*self.latents(self.X)))
        self.close_track()
        return e

    def op_llgrad(self):
        lam, amp, noi, mean = self.latents(self.X)
        res_o = O.nonstationary_loglike_grad(self.X, self.y, lam, amp, noi, mean=mean, discrete=self.disc)
        res = self.g.loglike_grad()
        e = abs(res[0] - res_o[0]) / (1 + abs(res_o[0]))
        for got, want in zip(res[1:], res_o[1:]):
            e = max(e, np.abs(got - want).max() / (1 + np.abs(want).max()) / 10)
        return e

    def op_track(self):
        if self.track is None:
            self.tXs = self.points(int(self.rng.choice([1, 31, 64, 100])))
            self.tlat = self.latents(self.tXs, noise=False)
            self.tcand = api.Candidates(self.tXs)
            self.track = api.GibbsTrack(self.g, self.tcand, *self.tlat)
            self.tcap = cap256(self.rows()) + 256
        self.check_track()

    def track_error(self):
        mu, var = self.track.moments()
        lam, amp, mean = self.tlat
        mu_o, var_o = O.nonstationary_mean_and_var(self.post, self.tXs, lam, amp, mean_s=mean, clip=False)
        return max(np.abs(mu - mu_o).max() / (1 + np.abs(mu_o).max()), np.abs(var - var_o).max() / amp.max() ** 2)

    def op_acqgrad(self):
        M = int(self.rng.choice([1, 3, 40, 224]))
        Xs, lam, amp, mean, mg = self.grad_args(M)
        best = float(np.median(self.y))
        acq, dacq = api.ngp_acq_ei_grad_set([[self.g]], Xs, lam[:, :, None], amp[:, None], None, None, [1.0], None, best, None,
                                            None if mean is None else mean[None, :], None if mg is None else mg[None])
        mu_o, var_o, dmu_o, dvar_o = O.nonstationary_mean_and_var_grad(self.post, Xs, lam, amp, None, None, mean, mg)
        vo = np.maximum(var_o, 0.0)
        want, dwant = O.expected_improvement_lin_grad([1.0], mu_o[None], vo[None], dmu_o[None], np.where(vo > 0, dvar_o, 0.0)[None], best)
        return max(np.abs(acq - want).max(), np.abs(dacq - dwant).max() / (1 + np.abs(dwant).max()) / 10)


for name, cls, salt in (("grad", GradSequence, 0), ("gibbs", GibbsSequence, 500)):
    if which not in ("both", name):
        continue
    worst = 0.0
    for case in range(ncases):
        seq = cls(case, np.random.default_rng(seed0 * 1000 + salt + case))
        worst = max(worst, seq.run())
        print(f"  {name} case {case} {seq.describe()} ops={seq.ops}: ok, worst error/tolerance so far {worst:.2e}, {time.time() - t_start:.0f} s",
              flush=True)
    print(f"fuzz_models {name}: {ncases} cases passed, worst error/tolerance {worst:.2e}", flush=True)
