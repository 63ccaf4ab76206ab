// mean_program.hpp — mean programs (boss_mean_t): the (x, θ) -> length-P closure of a Semiparametric model (the parametric model
// m(x; θ) of src/models/parametric.jl:31-34,186-207 under src/models/semiparametric.jl:79-92), or a plain prior mean x -> length-P
// vector (T = 0), traced into P straight-line programs over ONE shared input vector: inputs 0..d-1 are x, inputs d..d+T-1 are θ.
// Each output is a FitProg with d + T inputs, interpreted by fit_eval / fit_grad of fitness.hpp exactly as a fitness program is (the
// two functions the 50-digit tests pin); the reverse sweep's ∂/∂inputs is split into ∂m/∂x (first d) and ∂m/∂θ (last T).
#pragma once
#include "fitness.hpp"

namespace boss {

constexpr int MEAN_MAXIN = 32;                               // d + T; value ids stay below 32 + 32 + 64 = 128 < FIT_NOARG
constexpr int MEAN_MAX_WAVES = 4;

// LDS doubles per thread: y[d+T] | v[nI] for the values, | ay[d+T] | av[nI] behind them for the reverse sweep.
__host__ __device__ constexpr int mean_slots(int n_in, int nI, bool grad) { return (grad ? 2 : 1) * (n_in + nI); }
// One wave of the longest program with its reverse sweep: y[32] + v[64] + ay[32] + av[64] = 192 slots × 64 lanes × 8 bytes = 96 KiB
// (the values alone: 96 slots, 48 KiB).  A slot costs 512 bytes per wave, so up to 32 slots (a 3-instruction program of 6 inputs
// with its sweep is 18) keep 4 waves per workgroup within 64 KiB, 33..42 slots 3 waves, 43..64 slots 2, anything longer 1.
constexpr int MEAN_MAX_LDS = 64 * (int)sizeof(double) * mean_slots(MEAN_MAXIN, FIT_MAXI, true);

// What one evaluation writes, for the host interpreter and the kernel alike.  Block (s, p) sits at index p + P*s (layout 0, sample-major:
// mean_Xs S×P×M and mean_grad [s][p][d×M] of the acquisition calls) or s + S*p (layout 1, output-major: one output's blocks are the
// mean_X S×N and mean_jac of boss_gp_loglike_grad_batch_mean); a block holds m[n], jac_theta n×T column-major (j + n*t), jac_x d×n
// column-major (k + d*j).
__host__ __device__ inline size_t mean_block(int layout, int p, int s, int P, int S) {
    return layout == 0 ? (size_t)p + (size_t)P * s : (size_t)s + (size_t)S * p;
}

#ifdef __HIPCC__
// One thread per (point j, output p, parameter set s): grid = point tiles × P × min(S, 65535), sets beyond the grid's z extent in a
// stride loop.  The P programs lie in a device buffer; progs[blockIdx.y] is the same address for the whole workgroup (uniform loads).
// Values and adjoints live in strided LDS columns sized at launch from the actual programs (slot q of thread t at
// lds[q * blockDim.x + t]: a wave's accesses to one slot are 64 consecutive doubles), because inputs and results are indexed at run
// time, which in a private array means scratch memory.  nI_max: the longest of the P programs (the column layout is one for all).
// No atomics, no reductions: every result is one thread's, repeated calls agree bit for bit.  The stores of m and of jac_theta are
// contiguous in j; jac_x is stored d apart (d×n is small).  There is no workgroup barrier: threads behind the last point leave.
template <bool GRAD>
__global__ __launch_bounds__(64 * MEAN_MAX_WAVES) void mean_eval_kernel(const FitProg* __restrict__ progs, const double* __restrict__ X,
                                                                         const double* __restrict__ thetas, int n, int d, int T, int P, int S,
                                                                         int layout, int nI_max, double* __restrict__ m,
                                                                         double* __restrict__ jac_theta, double* __restrict__ jac_x) {
    extern __shared__ __attribute__((aligned(16))) char mean_lds_raw[];
    const int st = blockDim.x;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;                                      // (no workgroup barrier below)
    const int p = blockIdx.y;
    const FitProg& g = progs[p];
    const int n_in = d + T;
    double* cy = reinterpret_cast<double*>(mean_lds_raw) + threadIdx.x;
    double* cv = cy + (size_t)n_in * st;
    double* cay = cv + (size_t)nI_max * st;
    double* cav = cay + (size_t)n_in * st;
    for (int k = 0; k < d; ++k) cy[(size_t)k * st] = X[(size_t)j * d + k];
    for (int s = blockIdx.z; s < S; s += gridDim.z) {
        for (int t = 0; t < T; ++t) cy[(size_t)(d + t) * st] = thetas[(size_t)s * T + t];
        const size_t blk = mean_block(layout, p, s, P, S);
        double val;
        [[clang::always_inline]] val = fit_eval(g, cy, cv, st);   // (a call would bring a stack frame: scratch memory)
        m[blk * n + j] = val;
        if (GRAD) {
            [[clang::always_inline]] fit_grad(g, cy, cv, cay, cav, st);
            if (jac_theta)
                for (int t = 0; t < T; ++t) jac_theta[blk * n * T + (size_t)t * n + j] = cay[(size_t)(d + t) * st];
            if (jac_x)
                for (int k = 0; k < d; ++k) jac_x[blk * n * d + (size_t)j * d + k] = cay[(size_t)k * st];
        }
    }
}
#endif  // __HIPCC__

}  // namespace boss
