// fitness.hpp — fitness programs (boss_fit_t): a NonlinFitness closure traced into a straight-line program, its interpreter with
// reverse sweep (one __host__ __device__ function for the kernels, boss_fit_eval_host and stand-alone programs), and the
// Monte-Carlo Expected Improvement epilogues built on it (expected_improvement(::NonlinFitness), expected_improvement.jl:104-111).
#pragma once
#include "acq_kernels.hpp"

namespace boss {

// ------------------------------------------------------------------------------------------
// The program, as it travels in the kernel arguments (464 bytes).  Value ids: 0..P-1 inputs y_p, P..P+nC-1 constants,
// P+nC+i the result of instruction i; an instruction reads earlier ids only (validated by boss_fit_create).  b = FIT_NOARG on
// unary operations.
// ------------------------------------------------------------------------------------------
constexpr int FIT_MAXC = 32, FIT_MAXI = 64, FIT_NOARG = 255;
enum FitOp : int {
    FIT_ADD = 0, FIT_SUB, FIT_MUL, FIT_DIV, FIT_NEG, FIT_ABS, FIT_SQUARE, FIT_SQRT, FIT_EXP, FIT_LOG, FIT_SIN, FIT_COS, FIT_TANH,
    FIT_POW, FIT_MIN, FIT_MAX, FIT_NOPS,
    // acquisition programs only (boss_acqp_create; every other program keeps FIT_NOPS opcodes): Φ and φ of the standard normal
    FIT_NORMCDF = FIT_NOPS, FIT_NORMPDF, ACQ_NOPS
};
__host__ __device__ inline bool fit_is_unary(int op) { return (op >= FIT_NEG && op <= FIT_TANH) || op == FIT_NORMCDF || op == FIT_NORMPDF; }

// normcdf_dev / normpdf_dev (common.hpp) for host and device: the host interpreter computes the same expressions
__host__ __device__ inline double fit_normcdf(double z) { return 0.5 * erfc(-z * 0.7071067811865476); }
__host__ __device__ inline double fit_normpdf(double z) { return exp(-0.5 * z * z) * 0.3989422804014327; }

struct FitProg {
    int P, nC, nI, out;
    double c[FIT_MAXC];
    unsigned char op[FIT_MAXI], a[FIT_MAXI], b[FIT_MAXI];
};

// Slots are strided columns: slot q of this evaluation at base[q * st] (st = 1 on the host; the block's thread count in LDS, so
// that a wave's accesses to one slot hit 64 consecutive doubles).
__host__ __device__ inline double fit_get(const FitProg& g, const double* y, const double* v, int st, int id) {
    if (id < g.P) return y[(size_t)id * st];
    id -= g.P;
    if (id < g.nC) return g.c[id];
    return v[(size_t)(id - g.nC) * st];
}

// Forward pass: y[P] inputs (read), v[nI] instruction results (written).  Returns the program's value.
// MIN / MAX give NaN when either operand is NaN (Julia's min / max); everything else is what IEEE arithmetic and libm give.
// ACQ: the program may hold NORMCDF / NORMPDF (acquisition programs); the other interpreters are compiled without the two cases.
template <bool ACQ = false>
__host__ __device__ inline double fit_eval(const FitProg& g, const double* y, double* v, int st) {
    for (int i = 0; i < g.nI; ++i) {
        const double x = fit_get(g, y, v, st, g.a[i]);
        const double z = g.b[i] == FIT_NOARG ? 0.0 : fit_get(g, y, v, st, g.b[i]);
        double r;
        if (ACQ && g.op[i] >= FIT_NORMCDF) {
            v[(size_t)i * st] = g.op[i] == FIT_NORMCDF ? fit_normcdf(x) : fit_normpdf(x);
            continue;
        }
        switch (g.op[i]) {
            case FIT_ADD: r = x + z; break;
            case FIT_SUB: r = x - z; break;
            case FIT_MUL: r = x * z; break;
            case FIT_DIV: r = x / z; break;
            case FIT_NEG: r = -x; break;
            case FIT_ABS: r = fabs(x); break;
            case FIT_SQUARE: r = x * x; break;
            case FIT_SQRT: r = sqrt(x); break;
            case FIT_EXP: r = exp(x); break;
            case FIT_LOG: r = log(x); break;
            case FIT_SIN: r = sin(x); break;
            case FIT_COS: r = cos(x); break;
            case FIT_TANH: r = tanh(x); break;
            case FIT_POW: r = pow(x, z); break;
            case FIT_MIN: r = (x != x || z != z) ? x + z : (x <= z ? x : z); break;
            default: r = (x != x || z != z) ? x + z : (x >= z ? x : z); break;   // FIT_MAX
        }
        v[(size_t)i * st] = r;
    }
    return fit_get(g, y, v, st, g.out);
}

// Reverse sweep behind fit_eval on the same y / v: ay[P] receives ∂f/∂y, av[nI] is the instructions' adjoint scratch (both written
// here).  Conventions: ABS'(0) = 0; MIN / MAX pass the derivative to the FIRST operand on a tie; SQRT'(0) = +Inf; POW(a, b)
// differentiates in both operands, the ∂/∂b term dropped when b is a constant id (a < 0 with an integer constant exponent gives no
// NaN).  An instruction whose adjoint is exactly 0 is skipped (it passes nothing on, whatever its partial derivatives are).
// KZERO (kernel programs, kern_grad): a local partial that is exactly 0 passes 0 on as well, whatever the adjoint is (0·±Inf = 0).
// A kernel spelled through a distance — exp(-sqrt(r2)), sqrt(5 r2) — meets SQRT'(0) = +Inf times SQUARE' = 2·0 at coincident points
// (the Gram diagonal, a candidate on a training point); the 0 is the Matérn family's true derivative at r = 0 and what
// KernelFunctions / Distances return for the exponential kernel.
__host__ __device__ inline void fit_adj_add(const FitProg& g, double* ay, double* av, int st, int id, double w) {
    if (id < g.P) ay[(size_t)id * st] += w;
    else if (id >= g.P + g.nC) av[(size_t)(id - g.P - g.nC) * st] += w;
}
// ACQ as in fit_eval: NORMCDF' = φ, NORMPDF'(z) = −z φ(z).
template <bool KZERO, bool ACQ = false>
__host__ __device__ inline void fit_grad_sweep(const FitProg& g, const double* y, const double* v, double* ay, double* av, int st) {
    for (int p = 0; p < g.P; ++p) ay[(size_t)p * st] = 0.0;
    for (int i = 0; i < g.nI; ++i) av[(size_t)i * st] = 0.0;
    fit_adj_add(g, ay, av, st, g.out, 1.0);
    for (int i = g.nI - 1; i >= 0; --i) {
        const double w = av[(size_t)i * st];
        if (w == 0.0) continue;
        const int ia = g.a[i], ib = g.b[i];
        const double x = fit_get(g, y, v, st, ia);
        const double z = ib == FIT_NOARG ? 0.0 : fit_get(g, y, v, st, ib);
        const double r = v[(size_t)i * st];
        double da = 0.0, db = 0.0;
        if (ACQ && g.op[i] >= FIT_NORMCDF) {
            da = g.op[i] == FIT_NORMCDF ? fit_normpdf(x) : -x * r;
            fit_adj_add(g, ay, av, st, ia, w * da);
            continue;
        }
        switch (g.op[i]) {
            case FIT_ADD: da = 1.0; db = 1.0; break;
            case FIT_SUB: da = 1.0; db = -1.0; break;
            case FIT_MUL: da = z; db = x; break;
            case FIT_DIV: da = 1.0 / z; db = -r / z; break;
            case FIT_NEG: da = -1.0; break;
            case FIT_ABS: da = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); break;
            case FIT_SQUARE: da = 2.0 * x; break;
            case FIT_SQRT: da = 0.5 / r; break;
            case FIT_EXP: da = r; break;
            case FIT_LOG: da = 1.0 / x; break;
            case FIT_SIN: da = cos(x); break;
            case FIT_COS: da = -sin(x); break;
            case FIT_TANH: da = 1.0 - r * r; break;
            case FIT_POW:
                da = z * pow(x, z - 1.0);
                if (!(ib >= g.P && ib < g.P + g.nC)) db = r * log(x);
                break;
            case FIT_MIN: if (x <= z) da = 1.0; else db = 1.0; break;
            default: if (x >= z) da = 1.0; else db = 1.0; break;   // FIT_MAX
        }
        fit_adj_add(g, ay, av, st, ia, (KZERO && da == 0.0) ? 0.0 : w * da);
        if (ib != FIT_NOARG) fit_adj_add(g, ay, av, st, ib, (KZERO && db == 0.0) ? 0.0 : w * db);
    }
}
__host__ __device__ inline void fit_grad(const FitProg& g, const double* y, const double* v, double* ay, double* av, int st) {
    fit_grad_sweep<false>(g, y, v, ay, av, st);
}
// ... of a kernel program over u | v: ay[0..d) = ∂f/∂u, ay[d..2d) = ∂f/∂v
__host__ __device__ inline void kern_grad(const FitProg& g, const double* y, const double* v, double* ay, double* av, int st) {
    fit_grad_sweep<true>(g, y, v, ay, av, st);
}

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// Monte-Carlo EI epilogues.  One WAVE per candidate, lanes over the ε-samples: 224 ascent starts × 200 ε are 224 waves of 64 busy
// lanes (4 passes over k), spread over the chip, where a thread per candidate would be 4 waves.
//
// LDS: every thread owns a column of `slots` doubles, slot q at lds[q * blockDim.x + threadIdx.x] — the program's inputs and results
// are indexed at run time, which in a private array means scratch memory.  Layout of a column (mc_slots):
//     mu[P] | sd[P] | y[P] | v[nI]                        value kernel
//     ... | ay[P] | av[nI] | A[P] | B[P]                   gradient kernel (second set of slots for the reverse sweep, the sums)
// sized at launch from the program's P and instruction count (dynamic shared memory), so a short program keeps 4 waves per
// workgroup and several workgroups per CU.
//
// Summation order (fixed, no atomics: repeated calls agree bit for bit).  For one posterior sample, lane l adds its terms
// k = l, l + 64, l + 128, ... in ascending k into a private sum starting from 0; the 64 private sums are then combined by a butterfly
// over the lanes with xor masks 32, 16, 8, 4, 2, 1 (every lane ends with the same total: a + b == b + a); the total is divided by the
// number of ε-samples once.  Posterior samples are added in ascending s and divided by S once.
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int mc_slots(int P, int nI, bool grad) { return grad ? 6 * P + 2 * nI : 3 * P + nI; }
constexpr int MC_GRAD_MAX_LDS = 64 * (int)sizeof(double) * mc_slots(EI_MAXP, FIT_MAXI, true);   // one wave of the longest program: 112 KiB

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

// Feasibility product of candidate j for one sample (the loop of ei_value) and whether a variance is below the clip.
__device__ __forceinline__ double mc_feas(const double* __restrict__ mu, const double* __restrict__ var, int ldm, int j, const EiPar& par,
                                          bool& poison) {
    double fp = 1.0;
    for (int p = 0; p < par.P; ++p) {
        const double ym = (par.mode & 2) ? par.ymax[p] : INFINITY;
        const double m = mu[(size_t)p * ldm + j];
        double v = var[(size_t)p * ldm + j];
        if (v < 0.0) {
            if (v >= -MAX_NEG_VAR) v = 0.0;
            else poison = true;
        }
        if ((par.mode & 2) && !(isinf(ym) && ym > 0.0)) {
            const double s = sqrt(v);
            const double z = (s == 0.0 && ym == m) ? INFINITY : (ym - m) / s;
            fp *= normcdf_dev(z);
        }
    }
    return fp;
}

// (1/K) Σ_k max(0, f(μ + σ ⊙ ε_k) − best) of candidate j for one posterior sample, by the whole wave (every lane returns it).
// eps: the K columns (P doubles each) this sample uses.  GRAD: the column's A / B slots end up holding the wave totals
//   A_p = Σ_k 1[f_k > best] ∂f/∂y_p ,  B_p = Σ_k 1[f_k > best] ∂f/∂y_p ε_pk .
// NaN from the program propagates into the mean (max(0, NaN) is NaN, as in Julia) and contributes no gradient.
template <bool GRAD>
__device__ __forceinline__ double mc_ei_wave(const FitProg& g, const double* __restrict__ mu, const double* __restrict__ var, int ldm, int j,
                                             double best, const double* __restrict__ eps, int K, double* __restrict__ col, int st, int lane) {
    const int P = g.P, nI = g.nI;
    double* cmu = col;
    double* csd = cmu + (size_t)P * st;
    double* cy = csd + (size_t)P * st;
    double* cv = cy + (size_t)P * st;
    double* cay = cv + (size_t)nI * st;
    double* cav = cay + (size_t)P * st;
    double* cA = cav + (size_t)nI * st;
    double* cB = cA + (size_t)P * st;
    for (int p = 0; p < P; ++p) {
        double v = var[(size_t)p * ldm + j];
        if (v < 0.0) v = 0.0;                                // (below the clip the caller discards the result)
        cmu[(size_t)p * st] = mu[(size_t)p * ldm + j];
        csd[(size_t)p * st] = sqrt(v);
        if (GRAD) {
            cA[(size_t)p * st] = 0.0;
            cB[(size_t)p * st] = 0.0;
        }
    }
    double acc = 0.0;
    for (int k = lane; k < K; k += 64) {
        const double* e = eps + (size_t)k * P;
        for (int p = 0; p < P; ++p) cy[(size_t)p * st] = cmu[(size_t)p * st] + csd[(size_t)p * st] * e[p];
        const double f = fit_eval(g, cy, cv, st);
        const double imp = f - best;
        acc += (imp > 0.0) ? imp : ((imp != imp) ? imp : 0.0);
        if (GRAD && f > best) {
            fit_grad(g, cy, cv, cay, cav, st);
            for (int p = 0; p < P; ++p) {
                const double a = cay[(size_t)p * st];
                cA[(size_t)p * st] += a;
                cB[(size_t)p * st] += a * e[p];
            }
        }
    }
    if (GRAD)
        for (int p = 0; p < P; ++p) {
            cA[(size_t)p * st] = wave_sum(cA[(size_t)p * st]);
            cB[(size_t)p * st] = wave_sum(cB[(size_t)p * st]);
        }
    return wave_sum(acc) / (double)K;
}

// acq_sum[j] (+)= Σ_{s = s0 .. s1-1} acq_s(x_j): samples sstride apart behind mu / var (rows ldm apart), in ascending s.  S_total == 1
// (MAP): the one sample averages over all n_eps columns of eps; S_total > 1 (BI): sample s uses column s alone
// (expected_improvement.jl:87-90,108-111).  The mean over s, the mask and the arg-max follow in acq_epilogue_kernel.
constexpr int MC_MAX_WAVES = 4;
__global__ __launch_bounds__(64 * MC_MAX_WAVES) void ei_mc_accumulate_kernel(const double* __restrict__ mu, const double* __restrict__ var,
                                                                             size_t sstride, int ldm, int M, int s0, int s1, int S_total,
                                                                             EiPar par, FitProg g, const double* __restrict__ eps, int n_eps,
                                                                             double* __restrict__ acq_sum, int add) {
    extern __shared__ __attribute__((aligned(16))) char mc_lds_raw[];
    double* col = reinterpret_cast<double*>(mc_lds_raw) + threadIdx.x;
    const int st = blockDim.x, lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= M) return;                                      // (whole waves leave; there is no workgroup barrier below)
    double a = add ? acq_sum[j] : 0.0;
    if (par.mode != 0) {
        for (int s = s0; s < s1; ++s) {
            const double* mu_s = mu + (size_t)s * sstride;
            const double* var_s = var + (size_t)s * sstride;
            bool poison = false;
            const double fp = mc_feas(mu_s, var_s, ldm, j, par, poison);
            double as = fp;
            if (par.mode & 1) {
                const double ei = S_total == 1 ? mc_ei_wave<false>(g, mu_s, var_s, ldm, j, par.best, eps, n_eps, col, st, lane)
                                               : mc_ei_wave<false>(g, mu_s, var_s, ldm, j, par.best, eps + (size_t)s * g.P, 1, col, st, lane);
                as = (par.mode & 2) ? ei * fp : ei;
            }
            a += poison ? -INFINITY : as;
        }
    }
    if (lane == 0) acq_sum[j] = a;
}

// Acquisition and its gradient w.r.t. the candidate, averaged over S posterior samples: mu / var [s][p][M], dmu / dvar [s][p][d×M]
// (the layouts of ei_grad_set_kernel).  Per sample, with σ_p = sqrt(σ²_p), ∇σ_p = ∇σ²_p / (2σ_p) and ∇σ_p = 0 where the variance
// was clipped or is 0:   ∇EI = (1/K) Σ_p (A_p ∇μ_p + B_p ∇σ_p);   acq = EI·FP, ∇acq = ∇EI·FP + EI·∇FP (or EI, or FP, by mode) with
// FP and ∇FP as in ei_grad_point; masked candidates: 0 and 0; a variance below the clip in any sample: -Inf and gradient 0.  The x-dimension stays
// outside the Monte-Carlo loop: lane m (m, m + 64, ...) assembles coordinate m from the wave totals A, B.
__global__ __launch_bounds__(64 * MC_MAX_WAVES) void ei_mc_grad_set_kernel(const double* __restrict__ mu, const double* __restrict__ var,
                                                                           const double* __restrict__ dmu, const double* __restrict__ dvar,
                                                                           int M, int d, int S, EiPar par, FitProg g,
                                                                           const double* __restrict__ eps, int n_eps,
                                                                           const unsigned char* __restrict__ mask, double* __restrict__ acq,
                                                                           double* __restrict__ dacq) {
    extern __shared__ __attribute__((aligned(16))) char mc_lds_raw[];
    double* col = reinterpret_cast<double*>(mc_lds_raw) + threadIdx.x;
    const int st = blockDim.x, lane = threadIdx.x & 63;
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= M) return;
    const int P = par.P, mode = par.mode, nI = g.nI;
    double* gout = dacq + (size_t)j * d;
    for (int m = lane; m < d; m += 64) gout[m] = 0.0;
    if (mode == 0 || (mask && !mask[j])) {
        if (lane == 0) acq[j] = 0.0;
        return;
    }
    const double* cA = col + (size_t)(4 * P + 2 * nI) * st;
    const double* cB = cA + (size_t)P * st;
    const size_t pm = (size_t)P * M, dm = (size_t)d * M, pdm = pm * d;
    double asum = 0.0;
    bool any_poison = false;
    for (int s = 0; s < S; ++s) {
        const double* mu_s = mu + s * pm;
        const double* var_s = var + s * pm;
        const double* dmu_s = dmu + s * pdm;
        const double* dvar_s = dvar + s * pdm;
        bool poison = false;
        const double fp = mc_feas(mu_s, var_s, M, j, par, poison);
        double ei = 0.0;
        int K = 1;
        if (mode & 1) {
            K = S == 1 ? n_eps : 1;
            ei = mc_ei_wave<true>(g, mu_s, var_s, M, j, par.best, S == 1 ? eps : eps + (size_t)s * P, K, col, st, lane);
        }
        const double a = (mode & 1) ? ((mode & 2) ? ei * fp : ei) : fp;
        asum += poison ? -INFINITY : a;
        any_poison = any_poison || poison;
        if (poison) continue;
        for (int m = lane; m < d; m += 64) {
            double dei = 0.0, dfp = 0.0;
            for (int p = 0; p < P; ++p) {
                const double gm = dmu_s[(size_t)p * dm + (size_t)j * d + m];
                const double v = var_s[(size_t)p * M + j];
                const bool clipped = !(v > 0.0);
                const double gv = clipped ? 0.0 : dvar_s[(size_t)p * dm + (size_t)j * d + m];
                if (mode & 1) {
                    dei += cA[(size_t)p * st] * gm;
                    if (!clipped) dei += cB[(size_t)p * st] * (gv / (2.0 * sqrt(v)));
                }
                if (mode & 2) {
                    const double ym = par.ymax[p];
                    if (!(isinf(ym) && ym > 0.0) && !clipped) {
                        const double m_ = mu_s[(size_t)p * M + j], sd = sqrt(v);
                        const double t = (ym - m_) / sd;
                        const double dt = -gm / sd - (ym - m_) * gv / (2.0 * sd * v);
                        double others = 1.0;
                        for (int q = 0; q < P; ++q) {
                            if (q == p) continue;
                            const double yq = par.ymax[q];
                            if (isinf(yq) && yq > 0.0) continue;
                            double vq = var_s[(size_t)q * M + j];
                            if (vq < 0.0) vq = 0.0;
                            const double mq = mu_s[(size_t)q * M + j], sq = sqrt(vq);
                            const double tq = (sq == 0.0 && yq == mq) ? INFINITY : (yq - mq) / sq;
                            others *= normcdf_dev(tq);
                        }
                        dfp = __builtin_fma(others * normpdf_dev(t), dt, dfp);
                    }
                }
            }
            dei /= (double)K;
            gout[m] += (mode & 1) ? ((mode & 2) ? dei * fp + ei * dfp : dei) : dfp;
        }
    }
    if (lane == 0) acq[j] = asum / (double)S;
    for (int m = lane; m < d; m += 64) gout[m] = any_poison ? 0.0 : gout[m] / (double)S;   // (-Inf in any sample: the mean is -Inf, its gradient 0)
}
#endif  // __HIPCC__

}  // namespace boss
