/* bosship.h — C ABI of the MI355X-native GP-posterior + acquisition hot path for BOSS.jl.
 *
 * This is the drop-in boundary: the entry points are what a Julia `ccall`
 * layer behind BOSS's SurrogateModel / ModelFitter / AcquisitionMaximizer plugin API binds
 * (see INTEGRATION.md for the Julia stubs, and boss.jl_amd/ for the ctypes twin this pipeline
 * can execute).  Each function cites the reference code it replaces, relative to the
 * reference tree (soldasim/BOSS.jl v0.6.1).
 *
 * Conventions
 *   - all arrays are fp64, column-major, ONE OBSERVATION PER COLUMN (src/types/data.jl:10-12):
 *     X is d×N (x[k + d*j] = k-th coordinate of point j), candidates Xs are d×M.
 *   - the caller owns every host buffer; the library owns device memory behind opaque handles.
 *   - every function returns an int status (0 = BOSS_OK); no exception crosses the boundary;
 *     boss_last_error() returns a thread-local message for the last non-zero status.
 *   - the library is re-entrant across handles; one handle must not be used from two host
 *     threads at once (the reference calls its closures from Threads.@threads regions:
 *     src/utils/optim_multistart.jl:61-90, src/acquisition_maximizers/grid.jl:56-65).
 *   - there is NO CPU fallback: without a visible gfx950 device every compute entry point
 *     returns BOSS_E_NO_DEVICE.
 */
#ifndef BOSSHIP_H
#define BOSSHIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------ */
#define BOSS_OK            0
#define BOSS_E_INVALID     1   /* bad argument: the reference's @assert failures (gaussian_process.jl:227-233) */
#define BOSS_E_NO_DEVICE   2   /* no HIP device / HIP runtime error */
#define BOSS_E_NOT_PD      3   /* K + sigma^2 I not positive definite <-> LinearAlgebra.PosDefException */
#define BOSS_E_NEG_VAR     4   /* posterior variance < -1e-8 <-> DomainError from _clip_var (gaussian_process.jl:186-194) */
#define BOSS_E_NOT_FITTED  5   /* predict / acquisition on a handle that has no valid factorisation */
#define BOSS_E_ALLOC       6   /* device allocation failed */

/* ---- kernels: KernelFunctions.jl Matern32Kernel / Matern52Kernel (default, src/deprecated.jl:34) /
 *      SqExponentialKernel, always as alpha^2 * kernel ∘ ARDTransform(1 ./ lambda)
 *      (src/models/gaussian_process.jl:243) ------------------------------------------- */
#define BOSS_K_MATERN32 0
#define BOSS_K_MATERN52 1
#define BOSS_K_SQEXP    2

/* flags for boss_gp_update */
#define BOSS_FIT_DEFAULT   0
#define BOSS_FIT_NO_SYNC   1   /* enqueue only; logpdf_out is ignored, fetch later with boss_gp_sync */

typedef struct boss_gp   boss_gp_t;    /* one output slice's posterior: resident X, y, L, z (GaussianProcessPosterior, gaussian_process.jl:127-131) */
typedef struct boss_track boss_track_t; /* resident predictive state (V = L^-1 K*, mu, var) of one posterior at one candidate set */
typedef struct boss_cand boss_cand_t;  /* a resident batch of candidate points (the `xs` of SamplingAM.sample, sampling.jl:43-46) */

/* ---- library ---------------------------------------------------------------------- */
const char* boss_version(void);
const char* boss_last_error(void);
/* number of visible HIP devices (0 and BOSS_E_NO_DEVICE when none). */
int boss_device_count(int* n_devices_out);
/* run all work for `device` on the caller's HIP stream (e.g. torch's current stream); NULL restores the library's own stream. */
int boss_set_stream(int device, void* hip_stream);
/* block until everything enqueued on the device's stream has finished. */
int boss_device_sync(int device);

/* ---- posterior construction ---------------------------------------------------------
 * Replaces: posterior_gp / finite_gp / AbstractGPs.posterior (src/models/gaussian_process.jl:199-248)
 *           and logpdf(FiniteGP, y) (gp_data_loglike_slice, :269-280).
 *
 * boss_gp_create uploads the data of ONE output slice and keeps it resident:
 *   X        d×N, y N (row `slice` of ExperimentData.Y),
 *   discrete d flags or NULL — DiscreteKernel: flagged dims are rounded (half-to-even) in both
 *            kernel arguments (src/models/utils/kernels.jl:56-59).
 * boss_gp_update (re)builds the posterior for given hyper-parameters on the resident data:
 *   lengthscale d values, amplitude, noise_std: all must be >= 0 (else BOSS_E_INVALID); 1e-8 is
 *            ADDED to each (MIN_PARAM_VALUE, gaussian_process.jl:5,239-241);
 *   mean_X   N prior-mean values m(x_j) or NULL for the zero mean — user closures / the
 *            Semiparametric parametric mean (src/models/semiparametric.jl:79-84) are evaluated
 *            by the caller;
 *   logpdf_out  log marginal likelihood -(N log 2pi + logdet C + ||C.U'\(y-m)||^2)/2, may be NULL.
 * N is limited to 46080 observations per handle (BOSS_E_INVALID beyond).
 * On a non-PD matrix returns BOSS_E_NOT_PD, *logpdf_out = -Inf (what safe_data_loglike yields,
 * src/surrogate_model.jl:2-12) and the handle is left unfitted. */
int boss_gp_create(int device, int kernel, int d, int N, const double* X, const double* y,
                   const unsigned char* discrete, boss_gp_t** out);
int boss_gp_update(boss_gp_t* gp, const double* lengthscale, double amplitude, double noise_std,
                   const double* mean_X, int flags, double* logpdf_out);
/* wait for an update enqueued with BOSS_FIT_NO_SYNC; returns its status and logpdf. */
int boss_gp_sync(boss_gp_t* gp, double* logpdf_out);
/* one-shot convenience = create + update (the `boss_gp_fit` of SURVEY §8b). */
int boss_gp_fit(int device, int kernel, int d, int N, const double* X, const double* y,
                const double* mean_X, const double* lengthscale, double amplitude, double noise_std,
                const unsigned char* discrete, boss_gp_t** out, double* logpdf_out);
/* append-free refresh of the observations of a resident handle (same N): y only. */
int boss_gp_set_y(boss_gp_t* gp, const double* y);
/* Block Cholesky append.  Replaces: augment_dataset!(problem, x, y)
 * (src/types/problem.jl:191-198) followed by the model_posterior(problem) that
 * SequentialBatchAM's speculative loop recomputes from scratch for every selected point
 * (src/acquisition_maximizers/batch.jl:26-38), i.e. posterior_gp (gaussian_process.jl:199-211)
 * on the augmented data with the SAME hyper-parameters as the last boss_gp_update.
 * X_new is d×n column-major, y_new has n entries, mean_new is the prior mean at the new points
 * (n entries, or NULL for zero).  Only the 128-row blocks that contain new observations are
 * rebuilt (O(N^2) work per block instead of the O(N^3) re-factorisation); the result — factor,
 * z = L^{-1}(y-m), logpdf of all N+n observations — equals a fresh fit of the augmented data
 * to rounding.  The handle must be fitted; device storage grows as needed.  A posterior that was updated with a
 * prior mean (mean_X) requires mean_new (BOSS_E_INVALID otherwise).
 * From the second single-observation append after an update (the pattern of SequentialBatchAM and of
 * a BO loop that keeps its hyper-parameters) the handle keeps both inverse factors resident and an
 * append is one pass over each of them (rank-one append: L <- [L 0; l' d], L^-1 <- [L^-1 0; -w'/d 1/d]);
 * BOSS_WINV_AFTER=0 in the environment keeps every append on the block path. */
int boss_gp_append(boss_gp_t* gp, int n, const double* X_new, const double* y_new, const double* mean_new,
                   double* logpdf_out);
/* number of observations currently in the handle (after a boss_gp_append that failed part-way — n in 2..8 single
 * appends on resident inverse factors — it tells how many of them were taken). */
int boss_gp_n(const boss_gp_t* gp, int* n_out);
/* Reserve device storage for N_total observations (appends up to that size then need no
 * re-allocation).  Leaves the handle unfitted: follow with boss_gp_update. */
int boss_gp_reserve(boss_gp_t* gp, int N_total);
void boss_gp_free(boss_gp_t* gp);

/* Gradient of the log marginal likelihood w.r.t. the hyper-parameters.  Replaces: the
 * derivative of `loglike` (data_loglike, gaussian_process.jl:250-280) that OptimizationMAP's
 * optimiser obtains by automatic differentiation (src/model_fitters/optimization.jl:146-164).
 * Evaluated at the hyper-parameters of the last boss_gp_update on this handle:
 *   grad_out[0..d-1] = d logpdf / d lengthscale_m,  grad_out[d] = d/d amplitude,  grad_out[d+1] = d/d noise_std
 *   (d logpdf/d theta = 1/2 tr((a a' - K^-1) dK/dtheta), K^-1 = L^-T L^-1 formed on the device);
 *   logpdf_out (may be NULL) returns the value again.  grad_out holds the prior mean values fixed; the gradient
 *   through the mean (a Semiparametric model's theta) comes from boss_gp_loglike_grad_mean below.
 * Costs about one acquisition pass (triangular inverse) + a K = N syrk. */
int boss_gp_loglike_grad(boss_gp_t* gp, double* logpdf_out, double* grad_out);
/* boss_gp_loglike_grad plus d logpdf / d mean_X[j] = (K^-1 (y - m))_j, N values (N: the handle's current count, appended
 * points included).  With the Jacobian J of the mean values w.r.t. the parameters theta of a parametric mean
 * (src/models/semiparametric.jl:79-92), d logpdf / d theta = J' dmean_out.  logpdf_out and grad_out are
 * boss_gp_loglike_grad's; logpdf_out may be NULL.  Plain handles only (BOSS_E_INVALID for gradient-observation and
 * nonstationary handles: the latter have boss_ngp_loglike_grad's dmean_out); needs a fitted handle. */
int boss_gp_loglike_grad_mean(boss_gp_t* gp, double* logpdf_out, double* grad_out, double* dmean_out);

/* introspection for parity tests: lower Cholesky factor L (N×N column-major, upper part zeroed)
 * and z = L \ (y - m) (N). Either pointer may be NULL. */
int boss_gp_get_factor(const boss_gp_t* gp, double* L_out, double* z_out);

/* ---- gradient observations ----------------------------------------------------
 * Replaces: GradientGaussianProcess — model_posterior_slice (src/models/gradient_gp.jl:307-329),
 *           data_loglike (:367-397), mean / var / mean_and_var (:334-361).
 *
 * Every point carries its value and its gradient: n points give an n(1+d) system over the
 * observation ordering [y_1..n, dy/dx_1 (1..n), ..., dy/dx_d (1..n)] (_build_obs_vector, :288-302).
 * boss_ggp_create keeps one output slice resident:
 *   X   d×n,  y  n,  dY  d×n column-major (dY[l + d*j] = dy/dx_l at x_j — `data.dY[slice, :, :]`).
 * boss_ggp_update builds the augmented Gram matrix (_build_augmented_kernel, :175-210: value, first and
 * mixed second derivatives of the kernel, evaluated at (x_i, x_j + 1e-8) for coincident points; noise
 * (sigma+1e-8)^2 on the value block and (grad_noise_std+1e-8)^2 on the gradient blocks; the upper
 * triangle is the one that counts, `Symmetric(K)`), factorises it and returns
 *   logpdf_out = -(y~' K^-1 y~ + log|K| + n(1+d) log 2pi)/2.
 * The model's mean function is not used by the reference for this model and is not taken here.
 * The returned handle is a boss_gp_t: boss_gp_sync, boss_gp_predict (mu = k*'alpha, var = max(0, k(x,x) - |L^-1 k*|^2),
 * k* from _build_cross_cov :221-243; mean_Xs must be NULL), boss_gp_get_factor, boss_acq_ei, boss_acq_ei_moments
 * boss_gp_predict_grad and boss_acq_ei_grad (the gradients ForwardDiff pushes through :334-361 inside OptimizationAM,
 * src/acquisition_maximizers/optimization.jl:36,89-118; mean_Xs / mean_grad must be NULL; var is max(0, .), its gradient that of
 * the unclipped expression) and boss_gp_free work on it; boss_ggp_loglike_grad, boss_ggp_append, boss_ggp_reserve and
 * boss_ggp_track_create are its own forms of the likelihood gradient, of augment_dataset!, of reserve and of tracked candidates;
 * the entry points that assume value-only observations (boss_gp_update,
 * boss_gp_set_y, boss_gp_append, boss_gp_reserve, boss_gp_predict_cov, boss_gp_loglike_grad, boss_track_create) return
 * BOSS_E_INVALID; the posterior covariance of these handles is boss_ggp_predict_cov.
 * Limits: d <= 16, n(1+d) <= 46080. */
int boss_ggp_create(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY,
                    boss_gp_t** out);
int boss_ggp_update(boss_gp_t* gp, const double* lengthscale, double amplitude, double noise_std,
                    double grad_noise_std, int flags, double* logpdf_out);
/* data_loglike of the gradient-observation model with its gradient, as OptimizationMAP takes it through ForwardDiff
 * (src/model_fitters/optimization.jl:146-164 through gradient_gp.jl:367-397): at the parameters of the last boss_ggp_update,
 *   grad_out[d + 3] = d logpdf / d(lengthscale[0..d-1], amplitude, noise_std, grad_noise_std)
 * (= 1/2 sum_ab (a a' - K^-1)_ab dK_ab/dtheta over the matrix `cholesky(Symmetric(K))` sees, a = K^-1 y~; the lengthscale derivatives
 * of the second-derivative block need the third radial profile of the kernel).  logpdf_out may be NULL. */
int boss_ggp_loglike_grad(boss_gp_t* gp, double* logpdf_out, double* grad_out);
/* augment_dataset! (src/types/problem.jl:191-198) + the posterior at unchanged hyper-parameters: n_new further points with values
 * and gradients (X_new d×n_new, y_new n_new, dY_new d×n_new column-major).  The reference orders the observations
 * [y; dy/dx_1; ...; dy/dx_d], which would put new rows inside every block.  The handle keeps an ordering of its own instead: the
 * points present at boss_ggp_create in the reference's order, every later point's 1 + d rows (value first) behind them.  The
 * posterior, its logpdf, mean, variance and covariance are invariant under this symmetric permutation, and every entry is
 * evaluated with the row / column roles the reference gives it (the 1e-8 shift of coincident points depends on them).  So, as for
 * boss_gp_append, only the 128-row blocks that contain new rows are rebuilt on the device (O(N^2) work per block; more than four
 * such block rows, or all of them: the grown arrays are factorised again, on the device as well), at the hyper-parameters the
 * last boss_ggp_update staged on the device, verbatim.  Nothing of the handle's data travels to the host; device storage grows as
 * needed.  logpdf_out: logpdf of all n + n_new points.  Needs a fitted handle (BOSS_E_NOT_FITTED otherwise).  BOSS_E_NOT_PD
 * leaves the handle unfitted with the new points in it (logpdf -Inf).  Tracks of the handle (boss_ggp_track_create) survive an
 * append.  boss_gp_get_factor returns the factor in the handle's ordering. */
int boss_ggp_append(boss_gp_t* gp, int n_new, const double* X_new, const double* y_new, const double* dY_new, double* logpdf_out);
/* boss_gp_reserve for a gradient-observation handle, counted in POINTS: device storage for n_points_total points, i.e.
 * n_points_total (1 + d) rows, so appends up to that size need no re-allocation.  Leaves the handle unfitted: follow with
 * boss_ggp_update. */
int boss_ggp_reserve(boss_gp_t* gp, int n_points_total);

/* ---- nonstationary posteriors -----------------------------------------------------
 * Replaces: NonstationaryGP — NonstationaryKernel / gibbs_kernel (src/models/nonstationary_gp/nonstationary_gp.jl:61-107),
 *           finite_nongp (:153-196), model_posterior_slice (:153-157), data_loglike_slice (:237-245).
 *
 *   k(x, y) = ((a(x) + a(y))/2)^2 prod_i sqrt(2 l_i(x) l_i(y) / (l_i(x)^2 + l_i(y)^2)) exp(-(x_i - y_i)^2 / (l_i(x)^2 + l_i(y)^2)),
 *   noise s(x_j)^2 on the diagonal.  l(.), a(.), s(.) are the caller's latent models (ParametrizedGP posteriors or
 *   constants, _param_posterior_slice :198-212) evaluated on the host; they cross the ABI as arrays:
 *   lam_X d×N (column j = l(x_j)), amp_X N, noise_X N;  lam_Xs d×M, amp_Xs M at the candidates.
 *   Dims flagged discrete are rounded in both kernel arguments (make_discrete, :183-191); the latent models must
 *   then be evaluated at the rounded points as well.  No 1e-8 is added to these parameters (the reference adds none).
 * boss_ngp_update factorises and returns logpdf(FiniteGP, y); boss_ngp_predict is mean_and_var with _clip_var
 * (k(x*,x*) = a(x*)^2, +1e-18 jitter as for the plain model).  boss_gp_sync, boss_gp_set_y, boss_gp_get_factor,
 * boss_gp_free, boss_acq_ei_moments (EI on the predicted moments), boss_ngp_predict_grad and boss_acq_ei_grad_moments (their
 * gradients w.r.t. the candidates) work with these handles, boss_ngp_predict_cov is their mean_and_cov, boss_ngp_append /
 * boss_ngp_reserve / boss_ngp_track_create[_lat] their forms of append, reserve and tracked candidates; the other
 * boss_gp_* / boss_acq_* entry points and boss_track_create (boss_gp_predict_cov included) return BOSS_E_INVALID for them. */
int boss_ngp_create(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                    boss_gp_t** out);
int boss_ngp_update(boss_gp_t* gp, const double* lam_X, const double* amp_X, const double* noise_X,
                    const double* mean_X, int flags, double* logpdf_out);
/* augment_dataset! (src/types/problem.jl:191-198) for a fitted nonstationary posterior: n_new further observations with the latent
 * models' values AT THE NEW POINTS (lam_new d×n_new, amp_new, noise_new; mean_new when the posterior has a prior mean); the values
 * at the old points are the resident ones.  k(x_i, x_j) depends on the latent values at x_i and x_j alone, so no entry between two
 * old points changes and the new observations go to the end of the ordering: as for boss_gp_append, only the 128-row blocks that
 * contain new observations are rebuilt on the device (O(N^2) work per block; more than four such block rows, or all of them: the
 * grown arrays are factorised again, on the device as well), and the result — factor, z = L^{-1}(y-m), logpdf of all N+n_new
 * observations — equals a fresh fit of the augmented data to rounding.  Nothing of the handle's data travels to the host; device
 * storage grows as needed.  lam_new must be finite and > 0, amp_new and noise_new finite and >= 0 (BOSS_E_INVALID otherwise: the
 * handle stays as it was, fitted).  Needs a fitted handle (BOSS_E_NOT_FITTED otherwise).  BOSS_E_NOT_PD leaves the handle unfitted
 * (logpdf -Inf).  Tracks of the handle (boss_ngp_track_create) survive an append. */
int boss_ngp_append(boss_gp_t* gp, int n_new, const double* X_new, const double* y_new, const double* lam_new,
                    const double* amp_new, const double* noise_new, const double* mean_new, double* logpdf_out);
/* boss_gp_reserve for a nonstationary handle: device storage for N_total observations (the per-point latent arrays included), so
 * appends up to that size need no re-allocation.  Leaves the handle unfitted: follow with boss_ngp_update, whose lam_X / amp_X /
 * noise_X still have N columns (the reserved columns are padding). */
int boss_ngp_reserve(boss_gp_t* gp, int N_total);
/* data_loglike_slice (nonstationary_gp.jl:237-245) with its partial derivatives w.r.t. the latent models' VALUES at the training
 * points — what a gradient-based fitter's AD carries back to the latent models through finite_nongp (:183-196); the caller chains
 * them through its own latent models.  At the parameters of the last boss_ngp_update; every output may be NULL:
 *   dlam_out d×N (column j = d logpdf / d l(x_j), the layout of lam_X), damp_out N, dnoise_out N, dmean_out N (= K^-1 (y - m)).
 * x_dim <= 16. */
int boss_ngp_loglike_grad(boss_gp_t* gp, double* logpdf_out, double* dlam_out, double* damp_out, double* dnoise_out,
                          double* dmean_out);
int boss_ngp_predict(boss_gp_t* gp, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                     const double* mean_Xs, double* mu, double* var, long* bad_index);
/* mean_and_var of n nonstationary posteriors at the same M candidates in one call: the posteriors of the samples of a
 * Bayesian-inference fit (src/posterior.jl:15-19), every one with its own latent models.  lam_Xs d×M×n, amp_Xs M×n, mean_Xs NULL
 * or M×n (member after member); mu, var n×M (member after member) — the layout boss_acq_ei_moments takes for P = 1.  Equally
 * shaped handles (the members of a boss_ngp_fit_batch) are predicted in one launch, other lists member by member.  _clip_var as boss_ngp_predict: the first
 * member with a variance below -1e-8 fails the call with BOSS_E_NEG_VAR, bad_index_out = its first such candidate. */
int boss_ngp_predict_set(int n, boss_gp_t* const* gps, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                         const double* mean_Xs, double* mu, double* var, long* bad_index_out);
/* mean_and_var of a nonstationary posterior AND its gradient w.r.t. the candidates.
 * Replaces: the derivatives ForwardDiff pushes through nonstationary_gp.jl:153-196 inside OptimizationAM
 * (src/acquisition_maximizers/optimization.jl:36,89-118).  The candidate enters the Gibbs kernel directly and through the
 * latent l(x*), a(x*), whose Jacobians arrive evaluated like their values (the latent models are the caller's):
 *   dlam_Xs d×d×M, dlam_Xs[l + d*(m + d*j)] = d l_l / d x_m at candidate j, or NULL (constant lengthscales);
 *   damp_Xs d×M,   damp_Xs[m + d*j]         = d a / d x_m,                  or NULL (constant amplitude);
 *   mean_Xs M / mean_grad d×M prior mean and its gradient at the candidates, or NULL;
 *   mu, var (clipped like boss_ngp_predict), dmu, dvar d×M column-major (gradient of the UNclipped variance).
 * Dims flagged discrete get a zero explicit part; the caller passes zero Jacobian columns for them.  x_dim <= 16. */
int boss_ngp_predict_grad(boss_gp_t* gp, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                          const double* dlam_Xs, const double* damp_Xs, const double* mean_Xs, const double* mean_grad,
                          double* mu, double* var, double* dmu, double* dvar, long* bad_index);

/* ---- batched log-likelihood -----------------------------------------------------------
 * Replaces: the `loglike.(samples)` loop of SamplingMAP (src/model_fitters/sampling.jl:59-78) and the
 * per-sample likelihood calls of OptimizationMAP / TuringBI (src/model_fitters/optimization.jl:153-160,
 * ext/TuringExt.jl:78-86) for S hyper-parameter sets on the same (X, y) slice.
 *   lengthscales d×S (column s = set s), amplitudes S, noise_stds S,
 *   mean_X NULL, or N values shared by all sets (mean_stride = 0), or S×N with mean_stride = N.
 *   ll_out S (‑Inf where not PD), status_out S (BOSS_OK / BOSS_E_NOT_PD / BOSS_E_INVALID) or NULL. */
int boss_gp_loglike_batch(int device, int kernel, int d, int N, const double* X, const double* y,
                          const double* mean_X, int mean_stride, const unsigned char* discrete,
                          int S, const double* lengthscales, const double* amplitudes,
                          const double* noise_stds, double* ll_out, int* status_out);
/* The same with the gradient of every log-likelihood w.r.t. (lengthscale[d], amplitude, noise_std):
 * grad_out is (d+2)×S (column s = set s; zeros where the status is not BOSS_OK).  Replaces the S value-and-gradient
 * evaluations one round of a multistart OptimizationMAP makes (src/model_fitters/optimization.jl:146-164, gradients by
 * automatic differentiation there).  The factorisations run batched; d <= 32. */
int boss_gp_loglike_grad_batch(int device, int kernel, int d, int N, const double* X, const double* y,
                               const double* mean_X, int mean_stride, const unsigned char* discrete,
                               int S, const double* lengthscales, const double* amplitudes,
                               const double* noise_stds, double* ll_out, double* grad_out, int* status_out);
/* boss_gp_loglike_grad_batch plus the gradient through the prior mean.
 *   T, mean_jac: Jacobian of the mean values w.r.t. T mean parameters, N×T column-major per set,
 *                set after set (jac_stride = N*T), or ONE N×T matrix shared by all sets (jac_stride = 0,
 *                a mean that is linear in theta); T = 0 / mean_jac NULL: no fold.
 *   dmean_out  N×S or NULL: column s = d logpdf / d mean_X of set s = K^-1 (y - m);
 *   dtheta_out T×S or NULL: column s = mean_jac(s)' dmean(s), formed on the device.
 * ll_out, grad_out and status_out are boss_gp_loglike_grad_batch's for the same arguments in every bit.  A set whose
 * status is not BOSS_OK gets zeros in both columns.  mean_X may be NULL while mean_jac is given.  BOSS_E_INVALID for
 * T < 0, T > 0 with mean_jac NULL, a jac_stride other than 0 or N*T, dtheta_out with T = 0. */
int boss_gp_loglike_grad_batch_mean(int device, int kernel, int d, int N, const double* X, const double* y,
                                    const double* mean_X, int mean_stride, const unsigned char* discrete, int S,
                                    const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                    int T, const double* mean_jac, int jac_stride,
                                    double* ll_out, double* grad_out, double* dmean_out, double* dtheta_out, int* status_out);
/* The batched likelihood of the gradient-observation model: S parameter sets on one (X, y, dY) slice, arguments as in
 * boss_ggp_create (X d×n, y n, dY d×n column-major) and boss_ggp_update (every parameter gets +1e-8):
 *   lengthscales d×S (column s = set s), amplitudes S, noise_stds S, grad_noise_stds S;
 *   ll_out S (-Inf where not PD or invalid), status_out S (BOSS_OK / BOSS_E_NOT_PD / BOSS_E_INVALID for a negative parameter) or NULL.
 * The observation vector [y; dy/dx_1; ...; dy/dx_d] is built once; every launch covers the batch (grid.z = parameter set); the
 * augmented matrix of a set is bit for bit the one boss_ggp_update builds at those parameters.  S = 0 is a no-op.
 * Limits: d <= 16, n(1+d) <= 46080. */
int boss_ggp_loglike_batch(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY,
                           int S, const double* lengthscales, const double* amplitudes, const double* noise_stds,
                           const double* grad_noise_stds, double* ll_out, int* status_out);
/* The batched likelihood of the nonstationary model: S sets of latent values at the N training points, set after set:
 *   lam_X d×N×S (set s, column j = l(x_j)), amp_X N×S, noise_X N×S, taken as given (no 1e-8) and checked as boss_ngp_update
 *   checks them: a set holding a lengthscale that is not finite and > 0, or an amplitude or noise that is not finite and >= 0
 *   (negative, NaN, infinite), gets -Inf and BOSS_E_INVALID, the other sets are computed;
 *   mean_X NULL, or N values shared by all sets (mean_stride = 0), or S×N with mean_stride = N;
 *   discrete as in boss_ngp_create (the latent models are evaluated at the rounded points by the caller).
 *   ll_out S (-Inf where not PD or invalid), status_out S or NULL.  S = 0 is a no-op. */
int boss_ngp_loglike_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                           int S, const double* lam_X, const double* amp_X, const double* noise_X,
                           const double* mean_X, int mean_stride, double* ll_out, int* status_out);
/* The two models' batched likelihoods WITH their gradients: what a gradient-based fitter evaluates per round (one round of a
 * multistart OptimizationMAP, src/model_fitters/optimization.jl:146-164), all trial points of an output in one call.
 * boss_ggp_loglike_grad_batch: arguments, the +1e-8 rule, limits and validity checks of boss_ggp_loglike_batch; grad_out is
 *   (d+3)×S, column s = dl/d(lengthscale[d], amplitude, noise_std, grad_noise_std) of set s — what boss_ggp_loglike_grad returns
 *   after boss_ggp_update at those parameters, bit for bit.  A NULL grad_out is BOSS_E_INVALID.
 * boss_ngp_loglike_grad_batch: arguments and checks of boss_ngp_loglike_batch; the partial derivatives w.r.t. the latent values of
 *   every set as boss_ngp_loglike_grad returns them: dlam_out d×N×S (set after set, each in lam_X's layout), damp_out, dnoise_out,
 *   dmean_out N×S; each may be NULL.  d <= 16.
 * Both: ll_out and status_out as in the likelihood batches (the likelihoods are theirs bit for bit); a set that is invalid or not
 * positive definite gets -Inf, its status and zeros in every gradient output, the other sets are unaffected; S = 0 is a no-op.
 * The factorisations run batched, the gradient passes in groups of sets (grid.z = set) up to 2048 padded rows and set after set
 * over four streams above; one copy back and one synchronisation per chunk of sets.  A set's results do not depend on its position
 * in the batch or on its neighbours. */
int boss_ggp_loglike_grad_batch(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY,
                                int S, const double* lengthscales, const double* amplitudes, const double* noise_stds,
                                const double* grad_noise_stds, double* ll_out, double* grad_out, int* status_out);
int boss_ngp_loglike_grad_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                                int S, const double* lam_X, const double* amp_X, const double* noise_X,
                                const double* mean_X, int mean_stride, double* ll_out,
                                double* dlam_out, double* damp_out, double* dnoise_out, double* dmean_out, int* status_out);
/* S RESIDENT posteriors of one output slice out of ONE batched factorisation.
 * Replaces: the broadcast `model_posterior.(Ref(model), params, Ref(data))` over the S parameter samples of a Bayesian-inference
 * fit (src/posterior.jl:15-19; samples from ext/TuringExt.jl:88-107), i.e. S calls of posterior_gp (gaussian_process.jl:199-211)
 * on the same (X, y) slice.  Arguments as boss_gp_loglike_batch; X and y are uploaded once and shared by the S members.
 *   out S handles — ordinary boss_gp_t (predict, acquisition, gradients, update, append, free): each is freed with boss_gp_free;
 *       the shared device storage goes with the last one.  A member whose status is not BOSS_OK is returned unfitted.
 *   logpdf_out S log marginal likelihoods (-Inf where not PD) or NULL, status_out S (BOSS_OK / BOSS_E_NOT_PD / BOSS_E_INVALID) or NULL.
 * boss_acq_ei walks S > 1 equally shaped posteriors of an output in one prediction launch (grid = candidate tiles × samples). */
int boss_gp_fit_batch(int device, int kernel, int d, int N, const double* X, const double* y,
                      const double* mean_X, int mean_stride, const unsigned char* discrete,
                      int S, const double* lengthscales, const double* amplitudes,
                      const double* noise_stds, boss_gp_t** out, double* logpdf_out, int* status_out);
/* The same for the gradient-observation model and the nonstationary model: S RESIDENT posteriors out of one batched factorisation.
 * Replaces: model_posterior per sample of a Bayesian-inference fit (src/posterior.jl:15-19) over gradient_gp.jl:307-329 /
 * nonstationary_gp.jl:153-196.  Arguments, the +1e-8 rule and the validity checks as boss_ggp_loglike_batch /
 * boss_ngp_loglike_batch; out, logpdf_out, status_out as boss_gp_fit_batch (S >= 1).  The members are ordinary boss_ggp_* /
 * boss_ngp_* handles; a nonstationary member keeps its lam_X, amp_X, noise_X.  BOSS_E_ALLOC when the S factors do not fit
 * (nothing is left behind).  boss_acq_ei walks S > 1 gradient-model members of one fit in one prediction launch; nonstationary
 * members are predicted together by boss_ngp_predict_set. */
int boss_ggp_fit_batch(int device, int kernel, int d, int n, const double* X, const double* y, const double* dY,
                       int S, const double* lengthscales, const double* amplitudes, const double* noise_stds,
                       const double* grad_noise_stds, boss_gp_t** out, double* logpdf_out, int* status_out);
int boss_ngp_fit_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                       int S, const double* lam_X, const double* amp_X, const double* noise_X,
                       const double* mean_X, int mean_stride, boss_gp_t** out, double* logpdf_out, int* status_out);

/* ---- prediction -------------------------------------------------------------------------
 * Replaces: mean_and_var(post, X::Matrix) (gaussian_process.jl:174-178) =
 *   mu = m(X*) + K*' a ; V = C.U' \ K* ; var = k(x*,x*) - sum_i V_ij^2 + 1e-18 ; _clip_var.
 *   Xs d×M, mean_Xs M values m(x*_j) or NULL; mu, var: M each.
 * Returns BOSS_E_NEG_VAR and the first offending index in *bad_index (else -1) when a variance is
 * below -1e-8 (DomainError); mu/var are still written (var unclipped at the offending entries).
 * Calls with one to four candidates — the reference evaluates the acquisition one point at a time
 * (expected_improvement.jl:75,79) — are served from an explicit inverse factor that the handle builds
 * on the second such call after an update / append (≈1 ms once, N^2 doubles of extra device memory;
 * BOSS_WINV_AFTER=0 in the environment disables it). */
int boss_gp_predict(boss_gp_t* gp, int M, const double* Xs, const double* mean_Xs,
                    double* mu, double* var, long* bad_index);

/* Posterior moments AND their analytic gradients w.r.t. the candidate coordinates.
 * Replaces: the derivative of mean_and_var(post, x) that the reference obtains by pushing
 * ForwardDiff duals through AbstractGPs when OptimizationAM refines candidates
 * (src/acquisition_maximizers/optimization.jl:36 AutoForwardDiff, :89-118; acquisition closure
 * src/acquisitions/expected_improvement.jl:74-84):
 *   dmu[:,j]  = grad m(x*_j) + sum_i a_i grad k(x_i, x*_j),   a = (K+sigma^2 I)^-1 (y - m)
 *   dvar[:,j] = -2 sum_i w_ij grad k(x_i, x*_j),              w_j = (K+sigma^2 I)^-1 k*_j
 *   Xs d×M; mean_Xs M or NULL; mean_grad d×M (gradient of the prior mean at the candidates) or NULL;
 *   mu, var M each (var through _clip_var, as boss_gp_predict); dmu, dvar d×M column-major.
 * Dimensions flagged discrete are rounded inside the kernel (DiscreteKernel), their gradient is 0.
 * Costs about two boss_gp_predict passes (forward substitution + its adjoint). */
int boss_gp_predict_grad(boss_gp_t* gp, int M, const double* Xs, const double* mean_Xs, const double* mean_grad,
                         double* mu, double* var, double* dmu, double* dvar, long* bad_index);

/* Replaces: mean_and_cov(post, X::Matrix) / cov (gaussian_process.jl:163-167,180-184):
 *   Sigma = K** - V'V + 1e-18 I (M×M, column-major, full symmetric), diagonal through _clip_var.
 * Not on the acquisition path (EI only needs the diagonal); provided so the whole posterior API
 * of the plugin is served from the device-resident factor. */
int boss_gp_predict_cov(boss_gp_t* gp, int M, const double* Xs, const double* mean_Xs,
                        double* mu, double* cov, long* bad_index);

/* mean_and_cov of a gradient-observation posterior (boss_ggp_create handles).
 * Replaces: cov(post::GradientGPPosteriorSlice, X) (gradient_gp.jl:368-373) with its mean:
 *   Sigma_ij = (a+1e-8)^2 k(|(x_i - x_j) / (l+1e-8)|) - v_i'v_j,  v = L^-1 k*(x) (value-to-(values; gradients) cross-covariance),
 *   mu = k*' alpha.  No jitter, no clipping (the reference's cov does neither; its var clips to max(0, .)).
 * Sigma is M×M column-major, exactly symmetric (Sigma[i,j] and Sigma[j,i] are the same double).  1 <= M <= 32768.
 * Other handle kinds: BOSS_E_INVALID. */
int boss_ggp_predict_cov(boss_gp_t* gp, int M, const double* Xs, double* mu, double* cov);
/* mean_and_cov of a nonstationary posterior (boss_ngp_create handles), gaussian_process.jl:163-167,180-184 over the Gibbs kernel:
 *   Sigma = K**_Gibbs - V'V + 1e-18 I, diagonal through _clip_var (values from -1e-8 up to 0 become 0; below: BOSS_E_NEG_VAR,
 *   first such index in bad_index).  lam_Xs d×M, amp_Xs M are l(x*), a(x*) at the (rounded) candidates as for boss_ngp_predict,
 *   mean_Xs M the prior mean at the candidates or NULL; mu = m(x*) + K*'a.  Sigma M×M column-major, exactly symmetric.
 *   1 <= M <= 32768.  Other handle kinds: BOSS_E_INVALID. */
int boss_ngp_predict_cov(boss_gp_t* gp, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                         const double* mean_Xs, double* mu, double* cov, long* bad_index);

/* resident candidates (one upload, many acquisition passes / many posteriors) */
int boss_cand_create(int device, int d, int M, const double* Xs, boss_cand_t** out);
void boss_cand_free(boss_cand_t* cand);

/* ---- acquisition ------------------------------------------------------------------------
 * Replaces: the `vals = acq.(eachcol(xs)); argmax(vals)` loop of SamplingAM / GridAM
 * (src/acquisition_maximizers/sampling.jl:43-46,36-39; grid.jl:52-65) with acq built by
 * construct_acquisition(::ExpectedImprovement) (src/acquisitions/expected_improvement.jl:49-90):
 *   gps       P×S handles, gps[p + P*s] = output p of hyper-parameter sample s (S = 1 for MAP);
 *             the acquisition is averaged over s (:87-90);
 *   mean_Xs   NULL or P×M×S prior means at the candidates, index p + P*(j + M*s);
 *   fit_coefs P LinFitness coefficients (src/types/fitness.jl);
 *   y_max     P upper constraints, +Inf allowed (-> factor 1, src/utils/inf.jl), or NULL for
 *             `constraints === nothing`;
 *   has_best/best  best_so_far(...) (:134-140) — has_best = 0 means `nothing`;
 *   valid_mask M bytes or NULL: 0 -> acq = 0.0 (make_safe, :58-65: outside bounds / cons, evaluated
 *             by the caller because `cons` is a user closure);
 *   acq_out   M values or NULL; a candidate whose variance raises DomainError gets -Inf, as the
 *             reference's SafeFunction wrapper does (src/acquisition.jl:21-25);
 *   argmax_out / max_out  first index of the maximum (Julia argmax) over this batch and its value.
 * All handles and `cand` must live on the same device. */
int boss_acq_ei(int P, int S, boss_gp_t* const* gps, const boss_cand_t* cand,
                const double* mean_Xs, const double* fit_coefs, const double* y_max,
                int has_best, double best, const unsigned char* valid_mask,
                double* acq_out, long* argmax_out, double* max_out);

/* One BO iteration's model update AND its first acquisition in one call: the candidates' forward substitution rides along
 * the factorisation (csrc/rider.hpp) instead of starting when it has ended.
 * Replaces: the pair `estimate_parameters!` -> `maximize_acquisition` of src/bo.jl:30-48 for maximisers whose candidates
 * do not depend on the posterior (SamplingAM, src/acquisition_maximizers/sampling.jl:43-57; GridAM, grid.jl:52-65) —
 * i.e. boss_gp_update (posterior_gp, src/models/gaussian_process.jl:199-211) followed by boss_acq_ei (P = 1, S = 1:
 * mean_and_var :174-178 + construct_ei, src/acquisitions/expected_improvement.jl:68-101) on the SAME handle.
 *   gp, lengthscale, amplitude, noise_std, mean_X: as boss_gp_update;   cand: resident candidates on gp's device;
 *   mean_Xs  NULL or M prior means at the candidates;   fit_coef: the LinFitness coefficient of this output;
 *   y_max    the output's upper constraint (+Inf allowed: factor 1, src/utils/inf.jl); NaN = `constraints === nothing`
 *            (boss_acq_ei's y_max == NULL);   has_best / best, valid_mask: as boss_acq_ei;
 *   logpdf_out  the update's log marginal likelihood;   mu_out / var_out  M posterior moments (unclipped: what
 *       mean_and_var returns before _clip_var; the EI epilogue clips) or NULL;   acq_out  M values or NULL;
 *   argmax_out / max_out as boss_acq_ei;   fused_out (or NULL): 1 = the substitution rode along, 0 = the call ran the two
 *       phases one after the other (no resident chain for this size / device / stream, N <= 128, x_dim > 32, a fallback).
 * The numbers do not depend on which way the call went beyond the stated fp64 tolerance (the order of the floating-point
 * sums differs); repeated calls on one path are bit-identical.  Errors: as boss_gp_update (BOSS_E_NOT_PD leaves the handle
 * unfitted and the acquisition outputs untouched). */
int boss_gp_update_acq(boss_gp_t* gp, const double* lengthscale, double amplitude, double noise_std, const double* mean_X,
                       const boss_cand_t* cand, const double* mean_Xs, double fit_coef, double y_max, int has_best,
                       double best, const unsigned char* valid_mask, double* logpdf_out, double* mu_out, double* var_out,
                       double* acq_out, long* argmax_out, double* max_out, int* fused_out);

/* The same EI x feasibility epilogue (expected_improvement.jl:68-101,113-114) and arg-max, but
 * from posterior moments the caller already holds: mu/var are S×P×M, index j + M*(p + P*s)
 * (row p of sample s is what mean_and_var(post_s, Xs)[p, :] returns, src/posterior.jl:60-72).
 * Used when the P outputs are fitted on different GPUs and their (mu, var) rows were all-gathered
 * (one process per GPU; see boss.jl_amd/distributed.py).  var < -1e-8 poisons the candidate
 * with -Inf as in boss_acq_ei. */
int boss_acq_ei_moments(int device, int P, int S, int M, const double* mu, const double* var,
                        const double* fit_coefs, const double* y_max, int has_best, double best,
                        const unsigned char* valid_mask, double* acq_out, long* argmax_out,
                        double* max_out);

/* The chain rule of boss_acq_ei_grad (construct_ei, expected_improvement.jl:68-101,113-114) from moments and moment gradients the
 * caller already holds — boss_ngp_predict_grad per output of a nonstationary model, or outputs fitted on other ranks:
 *   mu / var P×M (row p at p*M; var clipped), dmu / dvar P blocks of d×M column-major;  the other arguments as boss_acq_ei_grad. */
int boss_acq_ei_grad_moments(int device, int P, int M, int d, const double* mu, const double* var, const double* dmu,
                             const double* dvar, const double* fit_coefs, const double* y_max, int has_best, double best,
                             const unsigned char* valid_mask, double* acq_out, double* dacq_out);

/* Acquisition value AND its gradient w.r.t. the candidates, for one hyper-parameter
 * sample (MAP).  Replaces: differentiating construct_acquisition(::ExpectedImprovement)
 * (src/acquisitions/expected_improvement.jl:49-101,113-114) with ForwardDiff inside OptimizationAM's
 * multistart refinement (src/acquisition_maximizers/optimization.jl:36,89-118):
 *   gps        P handles (one per output), all on one device;
 *   Xs         d×M candidates (host);  mean_Xs NULL or [p][M];  mean_grad NULL or [p][d×M];
 *   fit_coefs, y_max, has_best/best, valid_mask: as boss_acq_ei;
 *   acq_out    M values;  dacq_out d×M column-major (gradient of acq_out[j] w.r.t. candidate j).
 * The EI x feasibility chain rule runs on the device behind boss_gp_predict_grad's moment gradients. */
int boss_acq_ei_grad(int P, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                     const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best,
                     double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out);

/* boss_acq_ei_grad averaged over the S hyper-parameter samples of a Bayesian-inference fit, in ONE call: what OptimizationAM
 * differentiates when the model parameters are BI samples (src/acquisitions/expected_improvement.jl:87-90 inside
 * src/acquisition_maximizers/optimization.jl:89-118).
 *   gps        S×P handles, gps[p + P*s] as boss_acq_ei: plain (also semiparametric) or gradient-observation posteriors, all on one
 *              device with one x_dim; nonstationary handles: BOSS_E_INVALID (they bring latent values: boss_ngp_acq_ei_grad_set);
 *   mean_Xs    NULL or S×P×M, index j + M*(p + P*s);  mean_grad NULL or [s][p][d×M column-major] (both NULL for gradient observations);
 *   the other arguments as boss_acq_ei_grad.
 * For every sample s, (acq_s, grad acq_s) are exactly what boss_acq_ei_grad defines for its P handles; the outputs are
 * (sum_s acq_s)/S and (sum_s grad acq_s)/S, summed in ascending s and divided once: no atomics, repeated calls agree bit for bit.
 * S = 1 is boss_acq_ei_grad itself.  Equally shaped members (the members of boss_gp_fit_batch / boss_ggp_fit_batch calls, the
 * shape test of boss_acq_ei's set prediction) run forward substitution, adjoint substitution and accumulation with grid =
 * candidate tiles × members; any other list, BOSS_NO_SET_PREDICT=1 and a failed allocation of the set path go member by member
 * inside the same call (one candidate upload, one copy back).  Either path keeps a transposed copy of every member's factor on the
 * device (as boss_acq_ei_grad does per handle): when that cannot be allocated the call fails with BOSS_E_ALLOC; what the in-call
 * fallback saves is a failure of the set path's own scratch (V slabs, partial sums, descriptors).  P*S*M above 2^30: BOSS_E_INVALID.
 * After an error nothing stays enqueued. */
int boss_acq_ei_grad_set(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                         const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best,
                         double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out);

/* ---- fitness programs: Monte-Carlo EI of a nonlinear fitness on the device ------------------------------------------------
 * Replaces: expected_improvement(::NonlinFitness, ...) (src/acquisitions/expected_improvement.jl:104-111) inside
 * construct_acquisition (:49-90), and its ForwardDiff derivative inside OptimizationAM (src/acquisition_maximizers/
 * optimization.jl:36,100).  A closure cannot cross the C ABI; a straight-line arithmetic program can.
 *
 * boss_fit_t holds a validated program in SSA form over P inputs y_0..y_{P-1}:
 *   value ids 0..P-1 are the inputs, P..P+n_const-1 the constants, P+n_const+i the result of instruction i;
 *   code      3*n_instr ints, instruction i = (op, a, b) at code[3i..3i+2]; a and b are EARLIER value ids, b = -1 on unary ops;
 *   out_id    the value id that is the program's value (an input or a constant is allowed);
 *   limits    P <= 16, n_const <= 32, n_instr <= 64.
 * Opcodes (BOSS_FIT_*): ADD SUB MUL DIV (binary), NEG ABS SQUARE SQRT EXP LOG SIN COS TANH (unary), POW MIN MAX (binary).
 * Values are what IEEE fp64 arithmetic and libm give (LOG of a negative number is NaN); MIN / MAX return NaN when an operand is NaN.
 * Derivative conventions (reverse sweep, boss_fit_eval_host and the gradient kernels):
 *   ABS'(0) = 0;  MIN and MAX pass the derivative of the FIRST operand on a tie;  SQRT'(0) = +Inf, as IEEE gives;
 *   POW(a, b) differentiates in both operands; the d/db term is dropped when b is a constant id, so that a < 0 with an integer
 *   constant exponent gives no NaN;  an instruction whose adjoint is exactly 0 passes nothing on.
 * boss_fit_create returns BOSS_E_INVALID (with a message) for a forward or self reference, an unknown opcode, an exceeded limit, a
 * non-finite constant, b != -1 on a unary op, a bad out_id.  boss_fit_create / boss_fit_free / boss_fit_eval_host need no device.
 * boss_fit_eval_host: Y P×n column-major, f_out n values, df_out P×n (df/dy per column) or NULL — the interpreter function the
 * kernels call, run on the host. */
#define BOSS_FIT_ADD     0
#define BOSS_FIT_SUB     1
#define BOSS_FIT_MUL     2
#define BOSS_FIT_DIV     3
#define BOSS_FIT_NEG     4
#define BOSS_FIT_ABS     5
#define BOSS_FIT_SQUARE  6
#define BOSS_FIT_SQRT    7
#define BOSS_FIT_EXP     8
#define BOSS_FIT_LOG     9
#define BOSS_FIT_SIN    10
#define BOSS_FIT_COS    11
#define BOSS_FIT_TANH   12
#define BOSS_FIT_POW    13
#define BOSS_FIT_MIN    14
#define BOSS_FIT_MAX    15
typedef struct boss_fit boss_fit_t;
int boss_fit_create(int P, int n_const, const double* consts, int n_instr, const int* code, int out_id, boss_fit_t** out);
void boss_fit_free(boss_fit_t* fit);
int boss_fit_eval_host(const boss_fit_t* fit, int n, const double* Y, double* f_out, double* df_out);

/* The four acquisition calls with the analytic EI term of LinFitness replaced by the Monte-Carlo mean over eps-samples of a
 * fitness program.  Every argument is that of the call named beside it, except that `fit_coefs` is replaced by
 *   fit     the program (its P must equal the call's P);
 *   n_eps, eps   P×n_eps standard-normal draws, column-major (sample_eps, expected_improvement.jl:119), uploaded once per call.
 * EI term of one posterior sample, sigma = sqrt(clipped variance):
 *   S = 1 (MAP):  EI_j = (1/n_eps) sum_k max(0, f(mu_j + sigma_j .* eps_k) - best)                         (:104-107)
 *   S > 1 (BI):   sample s uses column s of eps alone (n_eps must equal S), the acquisition is the mean over s   (:87-90,108-111)
 * NaN from the program propagates (max(0, NaN) is NaN, as in Julia; the arg-max ranks NaN largest).  Everything else is as in the
 * analytic calls: has_best = 0 gives the feasibility product alone (the program is not evaluated), y_max = NULL and has_best = 0
 * give 0, a variance in [-1e-8, 0) is clipped to 0, below that the candidate is -Inf (gradient 0), +Inf in y_max is factor 1,
 * valid_mask zeroes, first-index arg-max.
 * Gradient, with grad sigma_p = grad var_p / (2 sigma_p), and 0 where the variance was clipped or is 0:
 *   grad EI_j = (1/n_eps) sum_p (A_p grad mu_p + B_p grad sigma_p),
 *   A_p = sum_k 1[f_k > best] df/dy_p,   B_p = sum_k 1[f_k > best] df/dy_p eps_pk,
 * and acq = EI*FP, grad acq = grad EI*FP + EI*grad FP as in boss_acq_ei_grad.
 * The sums over k follow a fixed tree (csrc/fitness.hpp), no atomics: repeated calls agree bit for bit.
 * BOSS_E_INVALID: fit's P differs from P, n_eps < 1, S > 1 with n_eps != S, P*n_eps > 2^20, a non-finite eps.
 *   boss_acq_ei_mc               [boss_acq_ei]               prediction on the device, then the Monte-Carlo epilogue, arg-max;
 *   boss_acq_ei_mc_moments       [boss_acq_ei_moments]       from host moments mu / var S×P×M;
 *   boss_acq_ei_mc_grad          [boss_acq_ei_grad_set]      value and gradient, S >= 1, the same handle kinds;
 *   boss_acq_ei_mc_grad_moments  [boss_acq_ei_grad_moments, with a leading S]  mu / var [s][p][M], dmu / dvar [s][p][d×M]; samples
 *                                summed in ascending s and divided once (nonstationary posteriors: boss_ngp_predict_grad_set output).
 * Not offered with a fitness program: the boss_multi_* calls, boss_acq_ei_tracks, boss_gp_update_acq. */
int boss_acq_ei_mc(int P, int S, boss_gp_t* const* gps, const boss_cand_t* cand, const double* mean_Xs, const boss_fit_t* fit,
                   int n_eps, const double* eps, const double* y_max, int has_best, double best,
                   const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out);
int boss_acq_ei_mc_moments(int device, int P, int S, int M, const double* mu, const double* var, const boss_fit_t* fit, int n_eps,
                           const double* eps, const double* y_max, int has_best, double best,
                           const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out);
int boss_acq_ei_mc_grad(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                        const double* mean_grad, const boss_fit_t* fit, int n_eps, const double* eps, const double* y_max,
                        int has_best, double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out);
int boss_acq_ei_mc_grad_moments(int device, int P, int S, int M, int d, const double* mu, const double* var, const double* dmu,
                                const double* dvar, const boss_fit_t* fit, int n_eps, const double* eps, const double* y_max,
                                int has_best, double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out);

/* ---- acquisition programs: a user-defined acquisition function on the device -------------------------------------------------
 * Replaces: construct_acquisition(acq::AcquisitionFunction, problem, options) -> (x -> Real) for a custom acquisition
 * (src/types/acquisition.jl:1-57) behind construct_safe_acquisition (src/acquisition.jl:21-25), and its ForwardDiff derivative
 * inside OptimizationAM.  The function of the posterior moments of one candidate travels as a straight-line program.
 *
 * boss_acqp_t holds a validated program in the form of boss_fit_t over 2P + Q inputs:
 *   value ids 0..P-1       mu_p, the posterior means of the P outputs;
 *   value ids P..2P-1      var_p, the posterior variances AFTER the clip below;
 *   value ids 2P..2P+Q-1   Q runtime scalars q, given with every call (best-so-far, beta_t, y_max: what changes per BO iteration);
 *   then the constants and the instruction results, as in boss_fit_t;
 *   limits    1 <= P <= 8, 0 <= Q <= 16, n_const <= 32, n_instr <= 64.
 * Opcodes: the BOSS_FIT_* ones and two unary ones that only boss_acqp_create accepts (every other *_create answers "unknown
 * opcode" for them):
 *   BOSS_ACQ_NORMCDF  Phi(z) = 0.5 erfc(-z / sqrt 2),          derivative phi(z);
 *   BOSS_ACQ_NORMPDF  phi(z) = exp(-z^2 / 2) / sqrt(2 pi),     derivative -z phi(z).
 * Derivative conventions: those of boss_fit_t.  boss_acqp_create refuses what boss_fit_create refuses.
 * boss_acqp_create / boss_acqp_free / boss_acqp_eval_host need no device.
 * boss_acqp_eval_host: the RAW program and its reverse sweep at n moment columns — mu, var P×n column-major, q Q scalars (may be
 * NULL when Q = 0), a_out n values, da_dmu / da_dvar P×n or NULL.  No clip and no mask are applied.
 *
 * The four acquisition calls.  Arguments are those of the EI call named beside each, with fit_coefs / y_max / has_best / best
 * replaced by the program, its scalars q (Q doubles, non-finite values allowed) and `outside`.  For candidate j and sample s:
 *   variance clip   a variance in [-1e-8, 0) enters the program as 0; a variance below -1e-8 in any output of any sample makes
 *                   the candidate's value -Inf and its gradient 0, and the program is not consulted for that sample;
 *   sample average  a_s = program(mu, var, q); S = 1: the value is a_0; S > 1: the a_s are added in ascending s and the sum is
 *                   multiplied by 1/S once.  No atomics: repeated calls agree bit for bit;
 *   mask            a candidate whose valid_mask byte is 0 gets the value `outside` (any double; -Inf is the value of
 *                   construct_safe_acquisition) and gradient 0;
 *   arg-max         first index of the maximum, NaN counts as the largest value;
 *   gradient        d acq / d x_m = (1/S) sum_s sum_p (abar_mu_p d mu_p / d x_m + abar_var_p d var_p / d x_m), abar from the reverse
 *                   sweep; p ascending, the mu term before the var term, s ascending; an output whose variance is <= 0 after
 *                   the clip contributes no var term.
 *   boss_acq_prog               [boss_acq_ei]               every handle kind boss_acq_ei takes, fitted sets included;
 *   boss_acq_prog_moments       [boss_acq_ei_moments]       from host moments mu / var S×P×M;
 *   boss_acq_prog_grad          [boss_acq_ei_grad_set]      value and gradient, S >= 1; program-kernel handles need boss_kgp_set_grad;
 *   boss_acq_prog_grad_moments  [boss_acq_ei_mc_grad_moments]  mu / var [s][p][M], dmu / dvar [s][p][d×M].
 * BOSS_E_INVALID: the program's P differs from P, q is NULL with Q > 0.
 * Not offered with an acquisition program: the boss_multi_* calls, boss_acq_ei_tracks, boss_gp_update_acq, the *_warp calls. */
#define BOSS_ACQ_NORMCDF 16
#define BOSS_ACQ_NORMPDF 17
typedef struct boss_acqp boss_acqp_t;
int boss_acqp_create(int P, int Q, int n_const, const double* consts, int n_instr, const int* code, int out_id, boss_acqp_t** out);
void boss_acqp_free(boss_acqp_t* acqp);
int boss_acqp_eval_host(const boss_acqp_t* acqp, int n, const double* mu, const double* var, const double* q, double* a_out,
                        double* da_dmu, double* da_dvar);
int boss_acq_prog(int P, int S, boss_gp_t* const* gps, const boss_cand_t* cand, const double* mean_Xs, const boss_acqp_t* acqp,
                  const double* q, const unsigned char* valid_mask, double outside, double* acq_out, long* argmax_out,
                  double* max_out);
int boss_acq_prog_moments(int device, int P, int S, int M, const double* mu, const double* var, const boss_acqp_t* acqp,
                          const double* q, const unsigned char* valid_mask, double outside, double* acq_out, long* argmax_out,
                          double* max_out);
int boss_acq_prog_grad(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs, const double* mean_grad,
                       const boss_acqp_t* acqp, const double* q, const unsigned char* valid_mask, double outside, double* acq_out,
                       double* dacq_out);
int boss_acq_prog_grad_moments(int device, int P, int S, int M, int d, const double* mu, const double* var, const double* dmu,
                               const double* dvar, const boss_acqp_t* acqp, const double* q, const unsigned char* valid_mask,
                               double outside, double* acq_out, double* dacq_out);

/* ---- mean programs: the Semiparametric model's parametric mean on the device, with its Jacobians ------------------------------
 * Replaces: the per-point calls of the parametric model m(x; θ) (src/models/parametric.jl:31-34,186-207) behind the Semiparametric
 * mean (src/models/semiparametric.jl:79-92) and of a GaussianProcess mean function (src/models/gaussian_process.jl:101-103), and the
 * ForwardDiff derivatives of both w.r.t. θ (OptimizationMAP, src/model_fitters/optimization.jl:146-164) and w.r.t. x (OptimizationAM,
 * src/acquisition_maximizers/optimization.jl:36,100).  A closure cannot cross the C ABI; straight-line programs can.
 *
 * boss_mean_t holds P validated programs, one per output, over ONE shared input vector: inputs 0..d-1 are x, inputs d..d+T-1 are θ
 * (T = 0: a plain mean function of x).  Each program is a fitness program (above) over d + T inputs — the same value ids, opcodes,
 * values and derivative conventions, the same interpreter — given as
 *   n_const[P], consts     the constants of output 0, then of output 1, ... (n_const[p] each);
 *   n_instr[P], code       3 ints per instruction, output after output;
 *   out_ids[P]             each output's value id;
 *   limits                 d >= 1, T >= 0, d + T <= 32, 1 <= P <= 16, per output 32 constants and 64 instructions.
 * boss_mean_create returns BOSS_E_INVALID for everything boss_fit_create refuses, the message naming the output and the instruction.
 * boss_mean_create / boss_mean_free / boss_mean_eval_host need no device.
 *
 * boss_mean_eval evaluates every output at the n columns of X (d×n column-major) for S parameter sets (thetas T×S column-major,
 * NULL iff T == 0) in ONE kernel launch — one thread per (point, output, set) — and returns on the host
 *   m          P·S blocks of n values;
 *   jac_theta  P·S blocks n×T column-major (j + n*t): ∂m/∂θ_t at point j, or NULL;
 *   jac_x      P·S blocks d×n column-major (k + d*j): ∂m/∂x_k at point j, or NULL
 * (both NULL: the reverse sweep is skipped).  Block (s, p) sits at
 *   layout = 0 (sample-major)   p + P*s: m is the mean_Xs S×P×M, jac_x the mean_grad [s][p][d×M] of boss_acq_ei_grad_set;
 *   layout = 1 (output-major)   s + S*p: one output's blocks are the mean_X S×N (mean_stride = N) and the mean_jac
 *                               (jac_stride = N*T) of boss_gp_loglike_grad_batch_mean.
 * NaN and Inf computed by a program are returned as computed.  No atomics: repeated calls agree bit for bit.
 * boss_mean_eval_host: the same arguments and layouts through the same interpreter functions on the host (tests).
 * BOSS_E_INVALID: n < 1, S < 1, NULL X or m, NULL thetas with T > 0, jac_theta with T == 0, layout not 0 or 1,
 * P·S·n·max(1, T, d) above 2^30.  BOSS_E_NO_DEVICE: boss_mean_eval without a GPU. */
typedef struct boss_mean boss_mean_t;
int boss_mean_create(int d, int T, int P, const int* n_const, const double* consts, const int* n_instr, const int* code,
                     const int* out_ids, boss_mean_t** out);
void boss_mean_free(boss_mean_t* mean);
int boss_mean_eval_host(const boss_mean_t* mean, int n, const double* X, int S, const double* thetas, int layout, double* m,
                        double* jac_theta, double* jac_x);
int boss_mean_eval(int device, const boss_mean_t* mean, int n, const double* X, int S, const double* thetas, int layout, double* m,
                   double* jac_theta, double* jac_x);

/* ---- warps: the input warp and the output transform of a TransformedModel as device programs ------------------------------------
 * Replaces: the per-column InputTransform.forward calls and the OutputTransform.forward calls per point of a TransformedModel's
 * posterior (src/models/transformed.jl:222-257,330-378), and the ForwardDiff derivatives OptimizationAM pushes through both closures
 * (src/acquisition_maximizers/optimization.jl:36).
 *
 * boss_warp_t holds validated COPIES of up to two programs, each given as a boss_mean_t with T == 0 (validation, limits, opcodes and
 * derivative conventions are those of mean programs; the handles may be freed afterwards):
 *   in_prog    NULL (identity) or x -> x_: d = d_user <= 16 inputs, d_model outputs (1..16; d_model may differ from d_user);
 *   out_prog   NULL (identity) or (mu_0..mu_{P-1}, sd_0..sd_{P-1}) -> (mu_0.., sd_0..): 2P inputs, 2P outputs, so P <= 8.  A joint
 *              transform is traced as it is; a per-output (sliced) one is packed into this form, its cross-derivatives exact zeros;
 *   P          the number of model outputs: 1..8 with an output program, 1..16 without.
 * BOSS_E_INVALID: both programs NULL, a program with T != 0, in_prog with more than 16 inputs, out_prog whose input or output count
 * is not 2P, P out of range.  boss_warp_create / boss_warp_free and the _host calls need no device.
 *
 * boss_warp_apply: Xs d_user×M column-major -> X_out d_model×M column-major (the layout boss_cand_create takes) and, unless NULL,
 * jac_out: per candidate j the block d_model×d_user column-major, jac_out[r + d_model*(k + d_user*j)] = d x__r / d x_k.  One thread
 * per candidate.  BOSS_E_INVALID: no input program, M < 1, NULL Xs or X_out, M·d_model·d_user above 2^30.
 *
 * boss_warp_moments: the model-space moments of S posterior samples to user space.
 *   mu_, var_      [s][p][M];
 *   dmu_, dvar_    [s][p][d_model×M] column-major per block (k' + d_model*j): gradients w.r.t. x_;
 *   jac            boss_warp_apply's jac_out, or NULL = the identity (then d_model = d_user);
 *   mu, var        [s][p][M];  dmu, dvar [s][p][d_user×M] (k + d_user*j): gradients w.r.t. x;
 *   the four gradient arrays are all NULL or all given; jac needs them, and they need jac when the warp has an input program.
 * Per sample and candidate, with sd_ = sqrt(var_) after a variance in [-1e-8, 0) is clipped to 0, and grad sd_ = grad var_/(2 sd_),
 * 0 where the variance was clipped or is 0 (the conventions of the Monte-Carlo section above):
 *   (mu, sd) = out_prog(mu_, sd_),  var = sd·sd whatever the sign of sd (transformed.jl:343,350);
 *   grad_{x_} out_r = sum_q d out_r/d mu_q grad mu_q + d out_r/d sd_q grad sd_q   (ascending q, the mu term first),
 *   grad_x = J' grad_{x_} (ascending k'),  grad var = 2 sd grad sd.
 * out_prog == NULL passes mu_ and var_ through bit for bit (no clip) and applies J' to dmu_ and dvar_.  NaN and Inf from a program
 * are returned as computed.  One thread per (candidate, sample, output row of 2P); no atomics: repeated calls agree bit for bit.
 * A variance below -1e-8 keeps the meaning it has for the caller: with bad_index given, the first one in memory order fails the call
 * with BOSS_E_NEG_VAR, *bad_index = its candidate, before any work (boss_gp_predict's convention); with bad_index NULL, the
 * sample's moments at that candidate pass through untouched with zero gradients, so that an acquisition epilogue behind this stage
 * makes the candidate -Inf (boss_acq_ei_grad_set's convention).
 * BOSS_E_INVALID: S < 1, M < 1, d_user outside 1..16 or different from the input program's, NULL moments, gradient arrays partly
 * given, jac without them or without an input program, S·P·M·max(d_model, d_user) above 2^30.
 * The _host calls run the same __host__ __device__ functions as the kernels on the host (tests). */
typedef struct boss_warp boss_warp_t;
int boss_warp_create(const boss_mean_t* in_prog, int P, const boss_mean_t* out_prog, boss_warp_t** out);
void boss_warp_free(boss_warp_t* warp);
int boss_warp_apply_host(const boss_warp_t* warp, int M, const double* Xs, double* X_out, double* jac_out);
int boss_warp_apply(int device, const boss_warp_t* warp, int M, const double* Xs, double* X_out, double* jac_out);
int boss_warp_moments_host(const boss_warp_t* warp, int S, int M, int d_user, const double* mu_, const double* var_,
                           const double* dmu_, const double* dvar_, const double* jac, double* mu, double* var, double* dmu,
                           double* dvar, long* bad_index);
int boss_warp_moments(int device, const boss_warp_t* warp, int S, int M, int d_user, const double* mu_, const double* var_,
                      const double* dmu_, const double* dvar_, const double* jac, double* mu, double* var, double* dmu,
                      double* dvar, long* bad_index);

/* The prediction and acquisition calls of a warped model in ONE call each: Xs (d_user×M, user space) goes up once, the input warp
 * writes a temporary candidate set on the device, the handles predict in model space exactly as the plain calls make them, the
 * moments of every sample go through boss_warp_moments' kernel where they lie, and the EI × feasibility epilogues of the plain
 * calls run on the user-space result — y_max, best and the arg-max are in user space, as in the reference, and for S > 1 the mean
 * over samples is taken on user-space EI (expected_improvement.jl:87-90 over TransformedPosteriors).  One copy back; no
 * intermediate result visits the host.
 *   gps        gps[p + P*s], fitted on model-space data: plain, semiparametric and gradient-observation handles as
 *              boss_acq_ei_grad_set takes them (nonstationary handles: BOSS_E_INVALID); their x_dim must be the warp's d_model;
 *   mean_Xs    the base model's prior mean at the WARPED points, [s][p][M], or NULL;
 *   mean_grad  its gradient w.r.t. x_ there, [s][p][d_model×M], or NULL (the layouts of boss_acq_ei_grad_set);
 *   mu, var    [s][p][M];  dmu, dvar [s][p][d_user×M];  acq_out M (may be NULL in boss_acq_ei_warp);  dacq_out d_user×M.
 * boss_warp_predict / boss_warp_predict_grad: a model variance below -1e-8 fails the call with BOSS_E_NEG_VAR, *bad_index = the
 * first such candidate; the acquisition calls make such a candidate -Inf with a zero gradient.
 * What the calls return, bit for bit: with an input program alone, boss_acq_ei_warp what boss_acq_ei returns on a candidate set
 * created from boss_warp_apply's X_out, boss_warp_predict what boss_gp_predict returns there; at S = 1, boss_warp_predict_grad
 * what boss_warp_apply -> boss_gp_predict_grad per output -> boss_warp_moments return, and boss_acq_ei_grad_warp what
 * boss_acq_ei_grad_moments makes of that.  In the acquisition calls equally shaped handles of S > 1 samples take the set launches
 * of the plain acquisition calls; the prediction calls go handle by handle, as boss_gp_predict[_grad] do.
 * Everything else (fit_coefs, y_max, has_best / best, valid_mask, arg-max rules) as in boss_acq_ei and boss_acq_ei_grad_set.
 * BOSS_E_INVALID: P differs from the warp's, handles of different devices or x_dim, x_dim different from d_model or above 16,
 * P·S·M·max(d_model, d_user) above 2^30.  After an error nothing stays enqueued and every handle stays usable. */
int boss_warp_predict(const boss_warp_t* warp, int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                      double* mu, double* var, long* bad_index);
int boss_warp_predict_grad(const boss_warp_t* warp, int P, int S, boss_gp_t* const* gps, int M, const double* Xs,
                           const double* mean_Xs, const double* mean_grad, double* mu, double* var, double* dmu, double* dvar,
                           long* bad_index);
int boss_acq_ei_warp(const boss_warp_t* warp, int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                     const double* fit_coefs, const double* y_max, int has_best, double best, const unsigned char* valid_mask,
                     double* acq_out, long* argmax_out, double* max_out);
int boss_acq_ei_grad_warp(const boss_warp_t* warp, int P, int S, boss_gp_t* const* gps, int M, const double* Xs,
                          const double* mean_Xs, const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best,
                          double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out);

/* Kernel programs: a user-defined covariance function k(u, v) as a traced straight-line program (KernelFunctions.Kernel /
 * CustomKernel(f), src/models/utils/kernels.jl:3-13, wrapped by finite_gp, gaussian_process.jl:239-243, as
 * (α+1e-8)² · with_lengthscale(kernel, λ+1e-8)).  The program has 2·d inputs — u[0..d) then v[0..d) — and otherwise the layout,
 * opcodes and limits (32 constants, 64 instructions) of a fitness program; d is 1..16.  boss_kern_create validates as
 * boss_fit_create does; boss_kern_create / boss_kern_free / boss_kern_eval_host need no device.
 * boss_kern_eval_host: U, V d×n column-major, k_out[j] = f(U[:, j], V[:, j]) — the interpreter function the kernels run.
 *
 * boss_kgp_create returns an ordinary posterior handle over such a program (the handle keeps a copy: the boss_kern_t may be freed
 * first).  With u_i = r(x_i) ⊘ (λ + 1e-8), r rounding the discrete dims half-to-even (DiscreteKernel, kernels.jl:56-59):
 *   K_ij = (α+1e-8)² f(u_i, u_j) + δ_ij (σ+1e-8)²,   K*_ij = (α+1e-8)² f(u_i, u*_j),   k(x*, x*) = (α+1e-8)² f(u*, u*),
 * the prior variance being EVALUATED per candidate, not taken as α².  The entry (i, j), i > j, of the matrix that is factorised is
 * f(u_j, u_i): cholesky(Symmetric(K)) reads the upper triangle.  logpdf, μ, σ² (+1e-18, _clip_var), BOSS_E_NOT_PD, BOSS_E_NEG_VAR
 * and prior means are those of boss_gp_create handles.  The kernels hold no atomics: repeated calls agree bit for bit.
 * Calls that take the handle: boss_gp_update (flags, logpdf_out as usual), boss_gp_sync, boss_gp_predict, boss_acq_ei (one-shot or
 * resident candidates, P outputs × S samples; the members of boss_kgp_fit_batch calls as a set, see there), boss_gp_set_y, boss_gp_n, boss_gp_get_factor, boss_gp_free.
 * Every other entry point that takes a boss_gp_t* returns BOSS_E_INVALID ("not available for program-kernel posteriors"), or, for
 * the boss_ggp_* / boss_ngp_* calls, their own "handle was not created by ..." refusal.
 * BOSS_E_INVALID: d outside 1..16, N < 1 or above 46080, NULL X, y or kern.
 *
 * Gradients are opt-in.  boss_kern_grad_host (no device): the program's value and all 2d partials of n pairs by one reverse sweep,
 * dU[m + d·j] = ∂f/∂u_m, dV[m + d·j] = ∂f/∂v_m at (U[:, j], V[:, j]); k_out may be NULL.  One convention beyond boss_fit_eval_host's
 * sweep: a local partial that is exactly 0 passes 0 on whatever the adjoint is (0·±Inf = 0), so a kernel spelled through a distance
 * (exp(-sqrt(r2)), sqrt(5 r2)) has finite partials at coincident points — the Matérn family's true 0, the exponential kernel's 0 of
 * KernelFunctions / Distances.
 * boss_kgp_set_grad(g, on) sets or clears a flag on a boss_kgp_create handle (BOSS_E_INVALID for any other handle), before or after
 * boss_gp_update.  While it is set, boss_gp_loglike_grad, boss_gp_loglike_grad_mean, boss_gp_predict_grad, boss_acq_ei_grad and
 * boss_acq_ei_grad_set (member by member) take the handle: ∂logpdf/∂(λ, α, σ) = ½ Σ G_ij ∂K_ij/∂·, G = a aᵀ − K⁻¹, with
 * ∂K_ij/∂λ_m = −α² (f_u,m u_i,m + f_v,m u_j,m)/(λ_m+1e-8), and at a candidate
 *   ∇μ_m = ∇m_m + Σ_i a_i α² f_v,m(u_i, u*)/(λ_m+1e-8),
 *   ∇σ²_m = [α² (f_u,m + f_v,m)(u*, u*) − 2 Σ_i w_i α² f_v,m(u_i, u*)]/(λ_m+1e-8),   w = K⁻¹ k*,
 * 0 in discrete dims.  A call that holds an unflagged program handle is refused as before.  Every other refusal stands.
 *
 * Appends and tracked candidates are opt-in as well.  boss_kgp_set_sequential(g, on) sets or clears a second flag, independent of
 * the gradient flag, on a boss_kgp_create handle or a member of boss_kgp_fit_batch (BOSS_E_INVALID for NULL and for any other
 * handle, "was not created by boss_kgp_create"), before or after boss_gp_update; nothing resident changes.  While it is set,
 * boss_gp_append (block rows, re-factorisation, or — from the second single observation on — the rank-one append on the resident
 * inverse factors, through device buffers), boss_gp_reserve and boss_track_create take the handle, and boss_track_sync /
 * boss_track_moments / boss_track_free and boss_acq_ei_tracks follow: the new Gram rows, the new column K(X, x_new), the new
 * diagonal entry k(x_new, x_new) + (σ+1e-8)² and the right-hand side k(x_r, x*) of a tracked row are the program's, evaluated on the
 * device; the tracked σ² is the unclipped k(x*, x*) − Σv² + 1e-18.  A member of a set is detached from its slab by its first append.
 * Without the flag these calls are refused as before ("program-kernel posteriors ... without boss_kgp_set_sequential"), and every
 * other refusal (boss_gp_update_acq, boss_gp_predict_cov, boss_multi_*, the warp, Monte-Carlo EI and latent-model calls,
 * boss_debug_rider_replay) holds for a flagged handle too. */
typedef struct boss_kern boss_kern_t;
int boss_kern_create(int d, int n_const, const double* consts, int n_instr, const int* code, int out_id, boss_kern_t** out);
void boss_kern_free(boss_kern_t* kern);
int boss_kern_eval_host(const boss_kern_t* kern, int n, const double* U, const double* V, double* k_out);
int boss_kgp_create(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                    const boss_kern_t* kern, boss_gp_t** out);
int boss_kern_grad_host(const boss_kern_t* kern, int n, const double* U, const double* V, double* k_out, double* dU, double* dV);
int boss_kgp_set_grad(boss_gp_t* g, int on);
int boss_kgp_set_sequential(boss_gp_t* g, int on);

/* S hyper-parameter sets of one output slice under ONE kernel program: `loglike.(samples)` of SamplingMAP
 * (src/model_fitters/sampling.jl:59-78) and the S posteriors of a Bayesian-inference fit (src/posterior.jl:15-19).
 * boss_kgp_loglike_batch: X d×N, y N, lengthscales d×S, amplitudes / noise_stds S, mean_X NULL, N values (mean_stride 0) or N×S
 * (mean_stride N); ll_out[s] is bit for bit the logpdf of boss_gp_update on a boss_kgp_create handle at the parameters of set s.
 * A set with invalid parameters (BOSS_E_INVALID) or a matrix that is not positive definite (BOSS_E_NOT_PD) gets -Inf and its
 * status in status_out (may be NULL); the other sets are computed.  The Gram matrices of all sets of a chunk (12 GiB of matrices)
 * are written by one launch.  S = 0 returns BOSS_OK and touches nothing.
 * boss_kgp_fit_batch: the arguments of boss_gp_fit_batch with the program in the kernel id's place (S = 0: BOSS_OK, nothing is
 * built).  out[s] are ordinary program-kernel handles — views into one slab, each with its own copy of the program — with the
 * factor, logpdf and predictions of a boss_kgp_create handle updated at set s; boss_gp_update on a member rewrites only that
 * member, boss_gp_set_y detaches it from the slab first, boss_kgp_set_grad works on a member, and whatever refuses a program-kernel
 * handle refuses a member with the same message.  n >= 2 members of such calls that have one shape and bytewise equal programs
 * (the S samples × P outputs of a model: one call per output over one boss_kern_t) are predicted by ONE set of launches in
 * boss_acq_ei (P × S) and the other value-only set calls; a list that mixes programs, or program and built-in handles, or holds a
 * boss_kgp_create handle or a detached member, goes member by member as before, and so do the gradient calls.
 * BOSS_E_INVALID (decided before a device is needed): NULL kern, d != the program's x_dim, S < 0, N < 1, NULL X or y, and for
 * S > 0 a NULL hyper-parameter array, ll_out or out. */
int boss_kgp_loglike_batch(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete,
                           const boss_kern_t* kern, int S, const double* lengthscales, const double* amplitudes,
                           const double* noise_stds, const double* mean_X, int mean_stride, double* ll_out, int* status_out);
int boss_kgp_fit_batch(int device, const boss_kern_t* kern, int d, int N, const double* X, const double* y, const double* mean_X,
                       int mean_stride, const unsigned char* discrete, int S, const double* lengthscales, const double* amplitudes,
                       const double* noise_stds, boss_gp_t** out, double* logpdf_out, int* status_out);

/* boss_ngp_predict_grad for n nonstationary posteriors at the same M candidates in ONE call, and the sample-averaged acquisition
 * gradient on top of it: boss_acq_ei_grad_set for NonstationaryGP posteriors (BI samples of a finite_nongp model under
 * OptimizationAM, src/acquisitions/expected_improvement.jl:87-90 inside src/acquisition_maximizers/optimization.jl:89-118).
 * Member after member, each member in the layout of the single-handle call (n = P*S, member i = p + P*s in the acquisition call):
 *   lam_Xs d×M×n, amp_Xs M×n         as boss_ngp_predict_set;
 *   dlam_Xs d×d×M×n or NULL          per member as boss_ngp_predict_grad (NULL: constant lengthscales for all members);
 *   damp_Xs d×M×n or NULL            per member as boss_ngp_predict_grad (NULL: constant amplitude for all members);
 *   mean_Xs M×n or NULL, mean_grad d×M×n column-major per member or NULL;
 *   mu, var n×M (var clipped as boss_ngp_predict_grad clips it), dmu, dvar n blocks of d×M column-major (dvar: gradient of the
 *   UNclipped variance).
 * boss_ngp_predict_grad_set: member i's outputs are what boss_ngp_predict_grad defines for gps[i] with member i's arguments; the
 * first member with a variance below -1e-8 fails the call with BOSS_E_NEG_VAR, bad_index_out = its first such candidate.
 * boss_ngp_acq_ei_grad_set: for every sample s, (acq_s, grad acq_s) is what boss_acq_ei_grad_moments returns on the P members'
 * boss_ngp_predict_grad results; the outputs are (sum_s acq_s)/S and (sum_s grad acq_s)/S, summed in ascending s and divided once
 * (no atomics: repeated calls agree bit for bit).  S = 1 is the P-output MAP case.  A variance below -1e-8 poisons the candidate
 * with -Inf (gradient 0) as in boss_acq_ei_grad_set.  Between the one upload and the one copy back everything stays on the device:
 * the Jacobians are folded in there.
 * Handles: from boss_ngp_create or boss_ngp_fit_batch (other kinds: BOSS_E_INVALID), fitted (BOSS_E_NOT_FITTED), one device, one
 * x_dim <= 16, the same discrete dimensions; lengthscales finite and > 0, amplitudes finite and >= 0 (BOSS_E_INVALID).
 * Limits: n*M <= 2^30 and n*M*x_dim^2 <= 2^27 (the Jacobian upload, 1 GiB), else BOSS_E_INVALID.
 * Equally shaped members (those of one boss_ngp_fit_batch; the shape test of boss_ngp_predict_set) run forward substitution,
 * adjoint substitution, accumulation and Jacobian fold with grid = candidate tiles x members; any other list,
 * BOSS_NO_SET_PREDICT=1 and a failed allocation of the set path's scratch go member by member inside the same call.  As
 * boss_acq_ei_grad_set, either path keeps a transposed copy of every member's factor (BOSS_E_ALLOC when that cannot be allocated).
 * After an error nothing stays enqueued and every handle stays usable. */
int boss_ngp_predict_grad_set(int n, boss_gp_t* const* gps, int M, const double* Xs, const double* lam_Xs, const double* amp_Xs,
                              const double* dlam_Xs, const double* damp_Xs, const double* mean_Xs, const double* mean_grad,
                              double* mu, double* var, double* dmu, double* dvar, long* bad_index_out);
int boss_ngp_acq_ei_grad_set(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* lam_Xs,
                             const double* amp_Xs, const double* dlam_Xs, const double* damp_Xs, const double* mean_Xs,
                             const double* mean_grad, const double* fit_coefs, const double* y_max, int has_best, double best,
                             const unsigned char* valid_mask, double* acq_out, double* dacq_out);

/* ---- resident latent models of a NonstationaryGP -------------------------------------------------
 * In the reference lam(x), alpha(x), sigma(x) of a NonstationaryGP are posteriors of latent ParametrizedGPs
 * (src/models/nonstationary_gp/nonstationary_gp.jl:200-214): a GP posterior mean m(x) pushed through Normal-cdf -> target quantile
 * -> activation (parametrized_gp.jl:91-134).  A boss_nlat_t holds the latent models of ONE output on the device and evaluates their
 * values and analytic Jacobians at candidates in one launch (latent_kernels.hpp): m = sum_i a_i k(x_i, x*), grad m = sum_i a_i grad
 * k(x_i, x*), then the transform and its chain rule in closed form.
 *   latent order q = 0..d-1 lengthscales, d amplitude, d+1 noise;
 *   a latent is a fitted plain handle (boss_gp_create + boss_gp_update, no prior mean, same device and d; other kinds
 *   BOSS_E_INVALID, unfitted BOSS_E_NOT_FITTED) or NULL = the constant given beside it (finite, taken as it is: no transform);
 *   noise is optional: noise_gp NULL and noise_const NaN = no noise model;
 *   target[q], target_par[2q], target_par[2q+1]: z = m | p0 + p1 m | exp(p0 + p1 m) | p0 + (p1 - p0) Phi(m);
 *   act[q], act_par[q]: z | log1p(exp z) + par (overflow-safe, derivative = sigmoid) | exp z;
 *   discrete: d flags or NULL — the nonstationary kernel's: candidates are rounded half-to-even in flagged dimensions before the
 *   lengthscale and amplitude latents see them and the Jacobian columns of those dimensions are zero; the noise latent sees the point
 *   as given (finite_nongp, nonstationary_gp.jl:192).
 * boss_nlat_create snapshots a = (K + sigma^2 I)^-1 y, the scaled training points, kernel, 1/lambda and amplitude of every latent
 * handle: afterwards the handles may be updated or freed.  Latents may have different N.  d <= 16.
 * Side effect on the latent handles: create forms a on each of them the way boss_gp_predict_grad does, i.e. it allocates that
 * handle's gradient workspace (the transposed factor, the inverted diagonal blocks and a: about N² doubles per latent handle) and makes
 * the handle's later boss_gp_update calls build the block inverses eagerly.  Nothing of it is shared with the object; a caller who
 * keeps the handles pays that memory and work until it frees them.
 * boss_nlat_eval: lam_out d×M, amp_out M, noise_out M or NULL, dlam_out d×d×M or NULL, damp_out d×M or NULL in the layouts
 * boss_ngp_predict_grad takes (dlam[l + d*(m + d*j)] = d lam_l / d x_m at candidate j).  A lengthscale that is not finite and > 0,
 * an amplitude or noise that is not finite and >= 0 fails the call with BOSS_E_INVALID, *bad_index = the first such candidate
 * (found by a flag the kernel sets).  No floating-point atomics: repeated calls agree bit for bit. */
#define BOSS_LT_NONE      0
#define BOSS_LT_NORMAL    1
#define BOSS_LT_LOGNORMAL 2
#define BOSS_LT_UNIFORM   3
#define BOSS_ACT_IDENTITY 0
#define BOSS_ACT_SOFTPLUS 1
#define BOSS_ACT_EXP      2
typedef struct boss_nlat boss_nlat_t;
int boss_nlat_create(int device, int d, boss_gp_t* const* lam_gps, const double* lam_const, boss_gp_t* amp_gp, double amp_const,
                     boss_gp_t* noise_gp, double noise_const, const int* target, const double* target_par, const int* act,
                     const double* act_par, const unsigned char* discrete, boss_nlat_t** out);
void boss_nlat_free(boss_nlat_t* lat);
int boss_nlat_eval(const boss_nlat_t* lat, int M, const double* Xs, double* lam_out, double* amp_out, double* noise_out,
                   double* dlam_out, double* damp_out, long* bad_index);

/* The nonstationary prediction calls with the latent values read from a boss_nlat_t on the device instead of host arrays: each
 * takes the latent object(s) where its array twin takes lam_Xs, amp_Xs[, dlam_Xs, damp_Xs] and is otherwise identical in arguments,
 * limits, error behaviour and outputs.  The latent kernel writes the very device buffers the array form uploads into, so a _lat
 * call returns bit for bit what its twin returns when fed the arrays boss_nlat_eval produces for the same candidates.  Set calls:
 * n = P*S handles and n latent objects, member i = p + P*s; the same shape test decides set path against member-by-member and
 * BOSS_NO_SET_PREDICT=1 has the same meaning.  A latent object whose discrete flags, device or d differ from the handle's, or an
 * invalid latent value at a candidate: BOSS_E_INVALID.  After an error nothing stays enqueued and every handle stays usable.
 * One limit is the _lat form's own: boss_ngp_predict_grad_lat refuses M·d² > 2^27 (BOSS_E_INVALID), the size of the device Jacobian
 * buffer the latent kernel fills, as the set calls of both forms do; boss_ngp_predict_grad, which reads its Jacobians from host
 * memory, has no such limit. */
int boss_ngp_predict_lat(boss_gp_t* gp, int M, const double* Xs, const boss_nlat_t* lat, const double* mean_Xs, double* mu,
                         double* var, long* bad_index);
int boss_ngp_predict_grad_lat(boss_gp_t* gp, int M, const double* Xs, const boss_nlat_t* lat, const double* mean_Xs,
                              const double* mean_grad, double* mu, double* var, double* dmu, double* dvar, long* bad_index);
int boss_ngp_predict_set_lat(int n, boss_gp_t* const* gps, int M, const double* Xs, boss_nlat_t* const* lats, const double* mean_Xs,
                             double* mu, double* var, long* bad_index_out);
int boss_ngp_predict_grad_set_lat(int n, boss_gp_t* const* gps, int M, const double* Xs, boss_nlat_t* const* lats,
                                  const double* mean_Xs, const double* mean_grad, double* mu, double* var, double* dmu, double* dvar,
                                  long* bad_index_out);
int boss_ngp_acq_ei_grad_set_lat(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, boss_nlat_t* const* lats,
                                 const double* mean_Xs, const double* mean_grad, const double* fit_coefs, const double* y_max,
                                 int has_best, double best, const unsigned char* valid_mask, double* acq_out, double* dacq_out);

/* ---- the nonstationary likelihood in whitened latent parameters -------------------------------------
 * A fitter of the reference does not move lam(x_j), alpha(x_j), sigma(x_j) but the whitened outputs y_eps of the latent
 * ParametrizedGPs (ParametrizedGPParams(X, mu, L, y_eps, lam), parametrized_gp.jl:49-77): the values at the data are
 * (L*y_eps + mu) pushed through Normal-cdf -> target quantile -> activation (parametrized_gp.jl:108-120; the closed forms of
 * boss_nlat_create).  A boss_nfit_t holds one output slice (X d×N, y, discrete, mean_X N values or NULL as boss_ngp_loglike_batch
 * takes them) and the latents' whitening resident, and evaluates data_loglike_slice (nonstationary_gp.jl:237-248) and its gradient
 * w.r.t. the whitened parameters of S parameter sets in one call: de-whitening, transform, Gibbs likelihood, its gradient and the
 * pull-back L'(c .* v') all on the device (nfit_kernels.hpp).
 *   factors    N×N×n_factors, column-major; the LOWER triangle of each is L of parametrized_gp.jl:200-202 (the rest is not read);
 *   factor_of  d+2 entries in latent order lam_0..lam_{d-1}, alpha, sigma: index into factors, or -1 = a scalar latent; latents
 *              with the same kernel and lengthscales share one uploaded factor;
 *   mu         N×(d+2), column q = mu of latent q (ignored for scalar latents), or NULL = zeros;
 *   target, target_par, act, act_par: d+2 (2(d+2)) entries as boss_nlat_create takes them, read for GP latents only.
 * theta T×S: column s holds the latents in order; a GP latent contributes its N values of y_eps, a scalar latent one number that is
 * its value at every point as given, without transform (_param_posterior_slice of a distribution latent,
 * nonstationary_gp.jl:200-207).  T = sum_q (N or 1) (boss_nfit_param_count).
 * Point j gets value j of its latent.  (The reference looks values up in a Dict keyed by the point, so of two identical columns
 * of X the last one's value would serve both; that is not emulated.)
 * boss_nfit_values: the lookup values in the layouts boss_ngp_update / boss_ngp_loglike_batch take (lam_out d×N×S, amp_out N×S,
 *   noise_out N×S), as computed (also for invalid sets); status_out S entries (BOSS_OK / BOSS_E_INVALID) or NULL.
 * boss_nfit_loglike_grad: ll_out[s] = the DATA term (params_loglike, logpdf(MvNormal(0, I), y_eps), stays with the caller);
 *   grad_out NULL or T×S: for a GP latent L_f'(c_q .* v'_q) with c_q the cotangent row of boss_ngp_loglike_grad (dlam rows, damp,
 *   dnoise), for a scalar latent sum_j c_q[j].  ll_out and status_out equal bit for bit what boss_ngp_loglike_batch returns for the
 *   arrays of boss_nfit_values: the device kernels write the very parameter blocks the array form uploads.  A set with a
 *   lengthscale that is not finite and > 0, an amplitude or noise that is not finite and >= 0, or a NaN in theta gets
 *   BOSS_E_INVALID, -Inf and a zero gradient column (a flag the kernel raises); not-PD sets as in boss_ngp_loglike_grad_batch; the
 *   other sets are unaffected.  A set's results do not depend on S, its position or its neighbours; no floating-point atomics.
 *   BOSS_MODEL_BATCH_CHUNK_MB chunks the call as it chunks the batched likelihoods; one upload of theta and one copy back of the
 *   gradients per chunk.  S = 0 is a no-op.  d <= 16.
 * Memory: the handle keeps every factor AND its transpose (the pull-back runs the same tile core on the transposed copy):
 * 2·8·Nk² bytes per factor, Nk = N rounded up to 64; per call 3·8·Nk·(columns rounded up to 32 per factor) bytes of chunk buffers,
 * columns = GP latents × sets of the chunk.  Arguments out of range, NULL arrays, unknown codes: BOSS_E_INVALID before any device
 * work; factors that do not fit: BOSS_E_ALLOC, nothing is left behind. */
typedef struct boss_nfit boss_nfit_t;
int boss_nfit_create(int device, int d, int N, const double* X, const double* y, const unsigned char* discrete, const double* mean_X,
                     int n_factors, const double* factors, const int* factor_of, const double* mu, const int* target,
                     const double* target_par, const int* act, const double* act_par, boss_nfit_t** out);
void boss_nfit_free(boss_nfit_t* fit);
int boss_nfit_param_count(const boss_nfit_t* fit, int* T_out);
int boss_nfit_values(boss_nfit_t* fit, int S, const double* theta, double* lam_out, double* amp_out, double* noise_out,
                     int* status_out);
int boss_nfit_loglike_grad(boss_nfit_t* fit, int S, const double* theta, double* ll_out, double* grad_out, int* status_out);

/* ---- tracked candidates -----------------------------------------------------------------------
 * SequentialBatchAM (src/acquisition_maximizers/batch.jl:26-38) re-evaluates the acquisition on
 * the whole candidate set after every speculative observation; with a FIXED candidate set (GridAM
 * points, or a seeded sample) the forward-substitution result V = C.U' \ K* can stay resident and
 * be EXTENDED by one row per appended observation (boss_gp_append) — an O(N M) update of mu and
 * var instead of the O(N^2 M) re-solve:
 *   boss_track_create   runs the prediction once and keeps V, mu, var (unclipped) on the device;
 *                       mean_Xs: prior mean at the candidates (M values) or NULL;
 *   boss_track_sync     brings the state up to the posterior's current N (no-op when in sync);
 *   boss_track_moments  copies mu / var (unclipped, like mean_and_var before _clip_var) of the
 *                       candidates [first, first+count) to the host (syncs first);
 *   boss_acq_ei_tracks  = boss_acq_ei on tracked states (tracks[p + P*s]; syncs them first).
 * A track is bound to the hyper-parameters of the boss_gp_update that preceded its creation:
 * after another boss_gp_update every call returns BOSS_E_INVALID (create a new track).  The
 * posterior handle must outlive its tracks. */
int boss_track_create(boss_gp_t* gp, const boss_cand_t* cand, const double* mean_Xs, boss_track_t** out);
/* The same for a nonstationary posterior (boss_ngp_append extends the state).  lam_Xs d×M and amp_Xs M are the latent models at
 * the candidates — evaluated by the caller at the ROUNDED candidates where dims are discrete, checked as boss_ngp_predict checks
 * them —, or are written on the device by a resident latent object (_lat; bit for bit the array form fed boss_nlat_eval's arrays,
 * the mismatch errors of boss_ngp_predict_lat).  The prediction runs once through the nonstationary path; the track keeps V, mu,
 * var (unclipped), the rounded candidates and l(x*), a(x*), from which every appended row's k(x_r, x*) is formed.  The track is
 * bound to the latent values of the boss_ngp_update that preceded its creation: after another boss_ngp_update every call returns
 * BOSS_E_INVALID.  boss_track_sync, boss_track_moments, boss_acq_ei_tracks and boss_track_free take these tracks as they take the
 * others.  Handles that are not nonstationary: BOSS_E_INVALID; unfitted: BOSS_E_NOT_FITTED; x_dim <= 16 (BOSS_E_INVALID beyond). */
int boss_ngp_track_create(boss_gp_t* gp, const boss_cand_t* cand, const double* lam_Xs, const double* amp_Xs, const double* mean_Xs,
                          boss_track_t** out);
int boss_ngp_track_create_lat(boss_gp_t* gp, const boss_cand_t* cand, const boss_nlat_t* lat, const double* mean_Xs,
                              boss_track_t** out);
/* The same for a gradient-observation posterior (boss_ggp_append extends the state, 1 + d rows per appended point).  The
 * prediction runs once through the model's own path; the track keeps V, mu, the raw candidates and the UNCLIPPED variance
 * k(x,x) - |v|^2 (a later row is subtracted from it); boss_track_moments and boss_acq_ei_tracks hand out the reference's
 * max(0, .) (gradient_gp.jl:343-361).  Bound to the hyper-parameters of the preceding boss_ggp_update like any track.  Handles
 * that are not gradient-observation posteriors: BOSS_E_INVALID; unfitted: BOSS_E_NOT_FITTED. */
int boss_ggp_track_create(boss_gp_t* gp, const boss_cand_t* cand, boss_track_t** out);
void boss_track_free(boss_track_t* track);
int boss_track_sync(boss_track_t* track);
int boss_track_moments(boss_track_t* track, int first, int count, double* mu, double* var);
int boss_acq_ei_tracks(int P, int S, boss_track_t* const* tracks, const double* fit_coefs, const double* y_max,
                       int has_best, double best, const unsigned char* valid_mask,
                       double* acq_out, long* argmax_out, double* max_out);

/* ---- several GPUs from ONE process (north_star: "shard embarrassingly across the 8 GPUs of one node with a
 * single RCCL allreduce over xGMI for the argmax") ---------------------------------------------------------------
 * What a Julia caller — no torch, no MPI — uses to spread the acquisition path over the GPUs of a node.  The devices
 * work concurrently (one host thread per device inside a call); the exchanges run over RCCL, which the library loads
 * at run time (dlopen librccl.so.1, ncclCommInitAll over all devices).  With one device and no RCCL the calls still work
 * (the exchange is the identity); with several devices and no RCCL boss_init fails (BOSS_E_NO_DEVICE).
 *
 * boss_init          enumerate the visible devices (BOSS_MAX_DEVICES in the environment caps the count), open a context
 *                    and a communicator on each.  Idempotent.  Replaces nothing in the reference (its parallelism is
 *                    Threads.@threads on the host: src/utils/optim_multistart.jl:61-90).
 * boss_comm_info     number of devices opened by boss_init and whether the exchanges run over RCCL.
 * boss_shutdown      destroy the communicators and exchange buffers (posterior handles are the caller's to free first). */
int  boss_init(int* n_devices_out);
int  boss_comm_info(int* n_devices_out, int* rccl_out);
void boss_shutdown(void);
/* The same hyper-parameters on G replicas of one posterior (gps[g] created by boss_gp_create on device g): every
 * device factorises concurrently; *logpdf_out from replica 0 (the factorisation is deterministic: all replicas agree). */
int boss_multi_gp_update(int G, boss_gp_t* const* gps, const double* lengthscale, double amplitude, double noise_std,
                         const double* mean_X, double* logpdf_out);
/* Candidates sharded over G devices (BASELINE config 3).  Replaces the same loop as boss_acq_ei
 * (src/acquisition_maximizers/sampling.jl:43-57) with the candidate columns split M/G:
 *   gps      G×S×P handles, gps[p + P*(s + S*g)] = replica on device g of output p, sample s;
 *   Xs       d×M candidates on the host; device g evaluates the contiguous, balanced shard g of the columns;
 *   mean_Xs, fit_coefs, y_max, has_best/best, valid_mask, acq_out (M values or NULL): as boss_acq_ei, for all M;
 *   argmax_out / max_out: the GLOBAL first-index arg-max — every device contributes its (max, global index) pair to ONE
 *   RCCL all-gather (16 bytes per rank; RCCL has no MAXLOC), reduced with Julia's argmax rules (ties: smaller index,
 *   NaN largest).  G must equal boss_init's count for the exchange to run over RCCL (a smaller G reduces on the host). */
int boss_multi_acq_ei(int G, int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                      const double* fit_coefs, const double* y_max, int has_best, double best,
                      const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out);
/* Outputs sharded (BASELINE config 4: "outputs sharded one-per-GPU"): gps[p + P*s] may live on ANY device opened by
 * boss_init (model_posterior_slice per output, src/models/gaussian_process.jl:133-141, fitted where it lives).  Each
 * owner predicts its (mu, var) rows for all M candidates; the rows travel in ONE RCCL all-reduce(sum) over zero-filled
 * blocks (exact), then the EI x feasibility epilogue and the arg-max run on the device of gps[0]
 * (expected_improvement.jl:68-90).  Arguments as boss_acq_ei with host candidates. */
// Resident candidate shards for boss_multi_acq_ei_cand: shard g (the balanced contiguous range of get_sample_counts,
// /root/reference/src/utils/sampling.jl:6-13) is uploaded to device g once; replaces the per-call `acq.(eachcol(xs))` operand of
// /root/reference/src/acquisition_maximizers/sampling.jl:43-57 when several acquisition calls share their candidates.
typedef struct boss_multi_cand boss_multi_cand_t;
int boss_multi_cand_create(int G, int d, int M, const double* Xs /*d×M*/, boss_multi_cand_t** out);
void boss_multi_cand_free(boss_multi_cand_t* cand);
int boss_multi_acq_ei_cand(int G, int P, int S, boss_gp_t* const* gps /*[G][S][P]*/, const boss_multi_cand_t* cand,
                           const double* mean_Xs /*P×M×S|NULL*/, const double* fit_coefs, const double* y_max, int has_best, double best,
                           const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out);
int boss_multi_acq_ei_outputs(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                              const double* fit_coefs, const double* y_max, int has_best, double best,
                              const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out);
/* Hyper-parameter samples sharded (BASELINE config 5): all P outputs of sample s live on one device, different samples
 * on different devices.  Every device sums acq_s(x_j) over ITS samples; ONE RCCL all-reduce(sum) of M doubles; the mean
 * over S (src/acquisitions/expected_improvement.jl:87-90), make_safe mask and arg-max on the device of sample 0. */
int boss_multi_acq_ei_samples(int P, int S, boss_gp_t* const* gps, int M, const double* Xs, const double* mean_Xs,
                              const double* fit_coefs, const double* y_max, int has_best, double best,
                              const unsigned char* valid_mask, double* acq_out, long* argmax_out, double* max_out);
/* boss_gp_loglike_batch with the S hyper-parameter sets split over devices 0..G-1 (contiguous, balanced); no collective:
 * every device writes its slice of ll_out / status_out. */
int boss_multi_loglike_batch(int G, int kernel, int d, int N, const double* X, const double* y, const double* mean_X,
                             int mean_stride, const unsigned char* discrete, int S, const double* lengthscales,
                             const double* amplitudes, const double* noise_stds, double* ll_out, int* status_out);

/* ---- measurement helpers (bench.py / profiles) ------------------------------------------ */
/* issue-rate microbenchmark of v_mfma_f64_16x16x4_f64: every SIMD of the device issues
 * `iters` x 16 independent MFMAs; returns the achieved TFLOP/s (calibrates the fp64 MFMA peak
 * that /opt/skills/guides/MI355X_MICROARCH.md does not list). */
int boss_bench_mfma_f64(int device, int iters, double* tflops_out);
/* per-kernel-class HIP-event timing: enable, run work, then read back (ms_total, launches). */
int boss_prof_enable(int device, int on);
int boss_prof_reset(int device);
int boss_prof_get(int device, const char* kernel_class, double* ms_total, long* launches);

#ifdef __cplusplus
}
#endif
#endif /* BOSSHIP_H */
