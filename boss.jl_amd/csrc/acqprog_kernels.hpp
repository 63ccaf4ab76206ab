// acqprog_kernels.hpp — acquisition programs (boss_acqp_t): a user-defined acquisition function traced into a FitProg over the
// posterior moments of one candidate, evaluated behind the prediction with the conventions of the built-in EI (ei_value /
// ei_grad_point): variance clip, average over the posterior samples in ascending order, domain mask, first-index arg-max.
#pragma once
#include "fitness.hpp"

namespace boss {

// The program's inputs: value ids 0..P-1 = μ_p, P..2P-1 = σ²_p (after the clip), 2P..2P+Q-1 = the runtime scalars q (FitProg::P is
// 2P + Q).  The scalars are the same for every candidate and travel in the kernel arguments.
constexpr int ACQP_MAXP = 8, ACQP_MAXQ = 16;
struct AcqpPar {
    int P, Q;
    double q[ACQP_MAXQ];
};

#ifdef __HIPCC__
// ------------------------------------------------------------------------------------------
// One THREAD per candidate (the program is evaluated once per candidate and sample; there is no ε-loop to spread over a wave).
// LDS: every thread owns a column of `slots` doubles, slot k at lds[k * blockDim.x + threadIdx.x], as in the Monte-Carlo kernels
// of fitness.hpp (inputs and results are indexed at run time, which in a private array means scratch memory):
//     y[2P+Q] | v[nI]                                      value kernel
//     y[2P+Q] | v[nI] | ay[2P+Q] | av[nI]                  gradient kernel (adjoints of the reverse sweep)
// Summation order (fixed, no atomics): the samples' values — and, per coordinate, the samples' gradients — are added in ascending s,
// the first sample starting the sum; the sum is multiplied by 1/S once.  Within a sample, coordinate m of the gradient is
//     Σ_p (ā_μp ∂μ_p/∂x_m + ā_vp ∂σ²_p/∂x_m)   in ascending p, the μ term before the σ² term, starting from 0;
// an output whose variance is <= 0 after the clip has no σ² term.
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int acqp_slots(int n_in, int nI, bool grad) { return (grad ? 2 : 1) * (n_in + nI); }
constexpr int ACQP_MAX_WAVES = 4;
constexpr int ACQP_GRAD_MAX_LDS = 64 * (int)sizeof(double) * acqp_slots(2 * ACQP_MAXP + ACQP_MAXQ, FIT_MAXI, true);   // one wave of the longest program: 96 KiB

// μ and the clipped σ² of candidate j for one sample into the column's input slots; true when a variance is below the clip
// (the candidate's value is then -Inf and the program is not consulted: ei_value's rule).
__device__ __forceinline__ bool acqp_load(const double* __restrict__ mu, const double* __restrict__ var, int ldm, int j, int P,
                                          double* __restrict__ cy, int st) {
    bool poison = false;
    for (int p = 0; p < P; ++p) {
        double v = var[(size_t)p * ldm + j];
        if (v < 0.0) {
            if (v >= -MAX_NEG_VAR) v = 0.0;
            else poison = true;
        }
        cy[(size_t)p * st] = mu[(size_t)p * ldm + j];
        cy[(size_t)(P + p) * st] = v;
    }
    return poison;
}

// acq_sum[j] (+)= Σ_{s = s0 .. s1-1} a_s(x_j): samples sstride apart behind mu / var (rows ldm apart), in ascending s.  The mean over
// s, the mask and the arg-max follow in acq_epilogue_kernel (mode 0, masked value `outside`).
__global__ __launch_bounds__(64 * ACQP_MAX_WAVES) void acqp_accumulate_kernel(const double* __restrict__ mu, const double* __restrict__ var,
                                                                              size_t sstride, int ldm, int M, int s0, int s1, AcqpPar ap,
                                                                              FitProg g, double* __restrict__ acq_sum, int add) {
    extern __shared__ __attribute__((aligned(16))) char acqp_lds_raw[];
    const int st = blockDim.x;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;                                      // (there is no workgroup barrier below)
    double* cy = reinterpret_cast<double*>(acqp_lds_raw) + threadIdx.x;
    double* cv = cy + (size_t)g.P * st;
    for (int k = 0; k < ap.Q; ++k) cy[(size_t)(2 * ap.P + k) * st] = ap.q[k];
    bool have = add != 0;
    double a = have ? acq_sum[j] : 0.0;
    for (int s = s0; s < s1; ++s) {
        const bool poison = acqp_load(mu + (size_t)s * sstride, var + (size_t)s * sstride, ldm, j, ap.P, cy, st);
        const double as = poison ? -INFINITY : fit_eval<true>(g, cy, cv, st);
        a = have ? a + as : as;
        have = true;
    }
    acq_sum[j] = a;
}

// Value and gradient w.r.t. the candidate, averaged over S samples: mu / var [s][p][M], dmu / dvar [s][p][d×M] (the layouts of
// ei_grad_set_kernel).  Masked candidates: `outside` and gradient 0; a variance below the clip in any sample: -Inf and gradient 0.
__global__ __launch_bounds__(64 * ACQP_MAX_WAVES) void acqp_grad_set_kernel(const double* __restrict__ mu, const double* __restrict__ var,
                                                                            const double* __restrict__ dmu, const double* __restrict__ dvar,
                                                                            int M, int d, int S, double inv_s, AcqpPar ap, FitProg g,
                                                                            const unsigned char* __restrict__ mask, double outside,
                                                                            double* __restrict__ acq, double* __restrict__ dacq) {
    extern __shared__ __attribute__((aligned(16))) char acqp_lds_raw[];
    const int st = blockDim.x;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    double* gout = dacq + (size_t)j * d;
    if (mask && !mask[j]) {
        acq[j] = outside;
        for (int m = 0; m < d; ++m) gout[m] = 0.0;
        return;
    }
    const int P = ap.P, nin = g.P, nI = g.nI;
    double* cy = reinterpret_cast<double*>(acqp_lds_raw) + threadIdx.x;
    double* cv = cy + (size_t)nin * st;
    double* cay = cv + (size_t)nI * st;
    double* cav = cay + (size_t)nin * st;
    for (int k = 0; k < ap.Q; ++k) cy[(size_t)(2 * P + k) * st] = ap.q[k];
    const size_t pm = (size_t)P * M, dm = (size_t)d * M, pdm = pm * d;
    double asum = 0.0;
    bool any_poison = false, gfirst = true;
    for (int s = 0; s < S; ++s) {
        const bool poison = acqp_load(mu + s * pm, var + s * pm, M, j, P, cy, st);
        const double as = poison ? -INFINITY : fit_eval<true>(g, cy, cv, st);
        asum = s == 0 ? as : asum + as;
        if (poison) {
            any_poison = true;
            continue;
        }
        fit_grad_sweep<false, true>(g, cy, cv, cay, cav, st);
        const double* dmu_s = dmu + s * pdm + (size_t)j * d;
        const double* dvar_s = dvar + s * pdm + (size_t)j * d;
        for (int m = 0; m < d; ++m) {
            double t = 0.0;
            for (int p = 0; p < P; ++p) {
                t += cay[(size_t)p * st] * dmu_s[(size_t)p * dm + m];
                if (cy[(size_t)(P + p) * st] > 0.0) t += cay[(size_t)(P + p) * st] * dvar_s[(size_t)p * dm + m];
            }
            gout[m] = gfirst ? t : gout[m] + t;
        }
        gfirst = false;
    }
    acq[j] = asum * inv_s;
    for (int m = 0; m < d; ++m) gout[m] = (any_poison || gfirst) ? 0.0 : gout[m] * inv_s;   // (-Inf in any sample: the mean is -Inf, its gradient 0)
}
#endif  // __HIPCC__

}  // namespace boss
