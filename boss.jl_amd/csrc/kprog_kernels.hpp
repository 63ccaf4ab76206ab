// kprog_kernels.hpp — program-kernel posteriors (boss_kgp_create): the covariance function is a user closure f(u, v) traced into a
// straight-line program (KernelFunctions.Kernel / CustomKernel(f), src/models/utils/kernels.jl:3-13, under finite_gp's
// (α+1e-8)² · with_lengthscale(kernel, λ+1e-8), gaussian_process.jl:239-243).  Two kernels write what the built-in radial profiles
// write for the plain model — the Gram matrix and the K* slabs — with the interpreter of fitness.hpp; everything behind them
// (factorisation, substitution, finish kernels) is the code every other model runs.
//
// Conventions: u = r(x) ⊘ (λ + 1e-8) come in scaled (scale_points_kernel / scale_cand_kernel; r rounds discrete dims);
//   K_ij  = (α+1e-8)² f(u_i, u_j) + δ_ij (σ+1e-8)²     the stored lower-triangle entry (i, j), i > j, is f(u_j, u_i):
//                                                      cholesky(Symmetric(K)) reads the upper triangle
//   K*_ij = (α+1e-8)² f(u_i, u*_j)
//   k(x*_j, x*_j) = (α+1e-8)² f(u*_j, u*_j)            EVALUATED per candidate (a dot-product kernel has no constant prior variance)
//
// LDS: as in mean_eval_kernel every thread owns a column of 2d + nI doubles (inputs u | v, then the instruction results), slot q at
// lds[q * blockDim.x + threadIdx.x] — the program indexes them at run time, which in a private array means scratch memory.  The
// workgroup is sized at launch (kprog_block, host_kprog.inc): as many of 4 waves as fit 64 KiB, so the longest program (96 slots,
// 48 KiB per wave) runs one wave per workgroup and a short one keeps four, several workgroups to a CU either way.  Every thread
// walks several entries in a stride loop.  The program travels in the kernel arguments.  No atomics: repeated calls agree bit for bit.
#pragma once
#include "fitness.hpp"

namespace boss {

constexpr int KERN_PROGRAM = 4;                               // internal id of a program kernel: no kappa_* function ever sees it
constexpr int KPROG_MAX_D = 16;                               // 2·d inputs <= MEAN_MAXIN = 32
constexpr int KPROG_MAX_WAVES = 4;
__host__ __device__ constexpr int kprog_slots(int d, int nI) { return 2 * d + nI; }

#ifdef __HIPCC__
// f(a, b) for the points a = A[·][ia], b = B[·][ib] (dimension-major, leading dimensions lda / ldb) in this thread's LDS column
__device__ __forceinline__ double kprog_pair(const FitProg& g, int d, const double* __restrict__ A, int lda, int ia,
                                             const double* __restrict__ B, int ldb, int ib, double* __restrict__ col, int st) {
    for (int k = 0; k < d; ++k) {
        col[(size_t)k * st] = A[(size_t)k * lda + ia];
        col[(size_t)(d + k) * st] = B[(size_t)k * ldb + ib];
    }
    [[clang::always_inline]] return fit_eval(g, col, col + (size_t)2 * d * st, st);
}

// One workgroup per 64×64 tile of the lower triangle (the grid, the padding rows and the unit diagonal of gibbs_gram_kernel):
// A[i + j·ld] for i >= j; rows / columns >= N are those of the identity.  hyp = {(α+1e-8)², (σ+1e-8)²} on the device.
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_gram_kernel(FitProg g, const double* __restrict__ Xsc, int d, int N, int Np,
                                                                          const double* __restrict__ hyp, double* __restrict__ A, int ld) {
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    const int st = blockDim.x, t = blockIdx.x;
    int bi = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
    while (bi * (bi + 1) / 2 > t) --bi;
    const int bj = t - bi * (bi + 1) / 2;
    const double amp2 = hyp[0], sig2 = hyp[1];
    for (int e = threadIdx.x; e < 64 * 64; e += st) {        // (a wave's 64 entries are one column of the tile: contiguous stores)
        const int i = bi * 64 + (e & 63), j = bj * 64 + (e >> 6);
        if (i < j) continue;
        double v;
        if (i < N && j < N) {
            v = amp2 * kprog_pair(g, d, Xsc, Np, j, Xsc, Np, i, col, st);   // entry (i, j), i >= j: f(u_j, u_i)
            if (i == j) v += sig2;
        } else {
            v = (i == j) ? 1.0 : 0.0;
        }
        A[(size_t)j * ld + i] = v;
    }
}

// K* where the substitution kernels take their right-hand side: out[tile][row][BN] (the layout of gibbs_kstar_kernel<BN>: the V
// slabs of predict_kernel<G, true>, or the residual array of the few-candidates path).  Grid (Np / 256, tiles); rows >= N and
// candidates >= M are 0.  The workgroups of row block 0 also write pvar[j] = (α+1e-8)² f(u*_j, u*_j) for their tile's candidates.
template <int BN>
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_kstar_kernel(FitProg g, const double* __restrict__ Xsc, int d, int N, int Np,
                                                                           const double* __restrict__ Csc, int Mp, int M, double amp2,
                                                                           double* __restrict__ out, double* __restrict__ pvar) {
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    const int st = blockDim.x, c0 = blockIdx.y * BN, rbase = blockIdx.x * 256;
    out += (size_t)blockIdx.y * Np * BN;
    for (int e = threadIdx.x; e < 256 * BN; e += st) {       // (consecutive threads: consecutive doubles of the slab)
        const int row = rbase + e / BN, c = e % BN, j = c0 + c;
        double v = 0.0;
        if (row < N && j < M) v = amp2 * kprog_pair(g, d, Xsc, Np, row, Csc, Mp, j, col, st);
        out[(size_t)row * BN + c] = v;
    }
    if (blockIdx.x == 0)
        for (int c = threadIdx.x; c < BN; c += st) {
            const int j = c0 + c;
            if (j < M) pvar[j] = amp2 * kprog_pair(g, d, Csc, Mp, j, Csc, Mp, j, col, st);
        }
}

// σ²(x*) = k(x*, x*) − Σv² + 1e-18: the finish kernels left −Σv² in var (their mode 2, as for the nonstationary model)
__global__ void kprog_var_kernel(double* __restrict__ var, const double* __restrict__ pvar, int M) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < M) var[j] = pvar[j] + var[j] + PREDICT_JITTER;
}
#endif  // __HIPCC__

}  // namespace boss
