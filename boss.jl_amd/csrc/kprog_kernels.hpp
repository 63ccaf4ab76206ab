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
//
// Many hyper-parameter sets at once (boss_kgp_loglike_batch, boss_kgp_fit_batch, predict_set_enqueue): kprog_gram_kernel takes the
// set in blockIdx.z over constant strides, kprog_scale_set_kernel writes every set's scaled points, and kprog_kstar_set_kernel /
// kprog_var_set_kernel are the set forms (grid.z / grid.y = member) of the K* and variance kernels — same bodies, same bits.
#pragma once
#include "fitness.hpp"

namespace boss {

constexpr int KERN_PROGRAM = 4;                               // internal id of a program kernel: no kappa_* function ever sees it
constexpr int KPROG_MAX_D = 16;                               // 2·d inputs <= MEAN_MAXIN = 32
constexpr int KPROG_MAX_WAVES = 4;
__host__ __device__ constexpr int kprog_slots(int d, int nI) { return 2 * d + nI; }
__host__ __device__ constexpr int kprog_grad_slots(int d, int nI) { return 2 * kprog_slots(d, nI); }   // values, then adjoints
constexpr int KPROG_GRAD_MAX_LDS = 64 * (int)sizeof(double) * kprog_grad_slots(KPROG_MAX_D, FIT_MAXI);   // one wave of the longest program: 96 KiB

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

// u = r(x) ⊘ (λ+1e-8) of nb parameter sets from the shared raw points (boss_kgp_loglike_batch, boss_kgp_fit_batch): grid.y = set, set b
// reads its 1/λ at par + b·sPar and writes Xsc + b·sX.  The product is scale_points_kernel's — the packed point (discrete dims
// rounded on the host) times the stored 1/λ —, so a set's scaled points are those of a handle updated at the same parameters.
__global__ void kprog_scale_set_kernel(const double* __restrict__ Xraw, double* __restrict__ Xsc, size_t sX, const double* __restrict__ par,
                                       size_t sPar, int d, int ldp) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ldp) return;
    for (int k = 0; k < d; ++k) Xsc[(size_t)b * sX + (size_t)k * ldp + j] = Xraw[(size_t)k * ldp + j] * par[(size_t)b * sPar + k];
}

// One workgroup per 64×64 tile of the lower triangle (the grid, the padding rows and the unit diagonal of gibbs_gram_kernel):
// A[i + j·ld] for i >= j; rows / columns >= N are those of the identity.  hyp = {(α+1e-8)², (σ+1e-8)²} on the device.
// blockIdx.z = parameter set (as aug_gram_kernel / gibbs_gram_kernel): set z reads its scaled points at Xsc + z·sX and its hyp at
// hyp + z·sHyp and writes A + z·bstride; a handle's update launches grid.z = 1 with zero strides.
// tile0: triangular index of the first tile (gram_kernel's): 0 for a whole matrix; the block rows of an append (append_rows_enqueue)
// launch the 4·kb + 3 tiles of block row kb from tile kb (2 kb + 1) — per tile a full build's arithmetic.
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_gram_kernel(FitProg g, const double* __restrict__ Xsc, size_t sX, int d, int N, int Np,
                                                                          const double* __restrict__ hyp, size_t sHyp, double* __restrict__ A, int ld,
                                                                          size_t bstride, int tile0) {
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    const int st = blockDim.x, t = tile0 + blockIdx.x;
    Xsc += (size_t)blockIdx.z * sX;
    hyp += (size_t)blockIdx.z * sHyp;
    A += (size_t)blockIdx.z * bstride;
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
// (one body for the single-handle and the set launch: `out` is the tile's slab, rblock / tile the workgroup's place in the grid)
template <int BN>
__device__ __forceinline__ void kprog_kstar_body(const FitProg& g, const double* __restrict__ Xsc, int d, int N, int Np,
                                                 const double* __restrict__ Csc, int Mp, int M, double amp2, double* __restrict__ out,
                                                 double* __restrict__ pvar, int rblock, int tile, double* __restrict__ col, int st) {
    const int c0 = tile * BN, rbase = rblock * 256;
    for (int e = threadIdx.x; e < 256 * BN; e += st) {       // (consecutive threads: consecutive doubles of the slab)
        const int row = rbase + e / BN, c = e % BN, j = c0 + c;
        double v = 0.0;
        if (row < N && j < M) v = amp2 * kprog_pair(g, d, Xsc, Np, row, Csc, Mp, j, col, st);
        out[(size_t)row * BN + c] = v;
    }
    if (rblock == 0)
        for (int c = threadIdx.x; c < BN; c += st) {
            const int j = c0 + c;
            if (j < M) pvar[j] = amp2 * kprog_pair(g, d, Csc, Mp, j, Csc, Mp, j, col, st);
        }
}
template <int BN>
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_kstar_kernel(FitProg g, const double* __restrict__ Xsc, int d, int N, int Np,
                                                                           const double* __restrict__ Csc, int Mp, int M, double amp2,
                                                                           double* __restrict__ out, double* __restrict__ pvar) {
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    kprog_kstar_body<BN>(g, Xsc, d, N, Np, Csc, Mp, M, amp2, out + (size_t)blockIdx.y * Np * BN, pvar, (int)blockIdx.x, (int)blockIdx.y, col,
                         (int)blockDim.x);
}

// K* of a SET of equally shaped program-kernel posteriors under ONE program, into the V slabs predict_kernel_set<G, true> reads
// (the layout of gibbs_kstar_set_kernel: member z, tile t at slab z·tiles + t, 32 candidates wide): grid = (256-row blocks,
// candidate tiles, members).  A member's scaled points, its scaled candidates (scale_cand_set_kernel) and α² come from its
// descriptor; its prior variances go to pvar + z·spv (the workgroups of row block 0).
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_kstar_set_kernel(FitProg g, int d, int N, int Np, int Mp, int M,
                                                                               const PredSet* __restrict__ sets, double* __restrict__ Vscratch,
                                                                               double* __restrict__ pvar, size_t spv) {
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    const PredSet ps = sets[blockIdx.z];
    kprog_kstar_body<32>(g, ps.Xsc, d, N, Np, ps.Csc, Mp, M, ps.amp2, Vscratch + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * Np * 32,
                         pvar + (size_t)blockIdx.z * spv, (int)blockIdx.x, (int)blockIdx.y, col, (int)blockDim.x);
}

// σ²(x*) = k(x*, x*) − Σv² + 1e-18: the finish kernels left −Σv² in var (their mode 2, as for the nonstationary model)
__global__ void kprog_var_kernel(double* __restrict__ var, const double* __restrict__ pvar, int M) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < M) var[j] = pvar[j] + var[j] + PREDICT_JITTER;
}
// ... of a set: grid.y = member, its σ² in its descriptor, its prior variances at pvar + y·spv
__global__ void kprog_var_set_kernel(const PredSet* __restrict__ sets, const double* __restrict__ pvar, size_t spv, int M) {
    const PredSet ps = sets[blockIdx.y];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < M) ps.var[j] = pvar[(size_t)blockIdx.y * spv + j] + ps.var[j] + PREDICT_JITTER;
}

// The new column of a rank-one append on resident inverse factors (boss_kgp_set_sequential, append_locked): column 0 of the 32-wide
// tile kstar_rows_kernel writes there for the built-in kernels, out[row·32] = (α+1e-8)² f(u_row, u_new) for row < N0 and 0 for
// N0 <= row < Np (winv_gemv_kernel<1> reads nothing else of the tile) — the entry kprog_kstar_body evaluates, row point first — and
// kself[0] = (α+1e-8)² f(u_new, u_new), the prior variance the new diagonal entry starts from.  u_new is candidate 0 of Csc [d][Mp].
// One row per thread: kprog_kstar_kernel<32> on a one-candidate block keeps 2 lanes of every wave busy (measured: 0.96 ms per
// append at N = 4096, d = 8, 31 instructions, against 0.14 ms with this kernel).
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_col_kernel(FitProg g, const double* __restrict__ Xsc, int d, int N0, int Np,
                                                                         const double* __restrict__ Csc, int Mp, double amp2,
                                                                         double* __restrict__ out, double* __restrict__ kself) {
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    const int st = blockDim.x, row = blockIdx.x * st + threadIdx.x;
    if (row < Np) out[(size_t)row * 32] = row < N0 ? amp2 * kprog_pair(g, d, Xsc, Np, row, Csc, Mp, 0, col, st) : 0.0;
    if (row == 0) kself[0] = amp2 * kprog_pair(g, d, Csc, Mp, 0, Csc, Mp, 0, col, st);
}

// Tracked candidates of a program-kernel posterior (boss_kgp_set_sequential): the right-hand sides of up to TRACK_ROWS appended rows,
// rhs[tile][q][32] = (α+1e-8)² f(u_{N0+q}, u*_j) for q < n — row point first, the entry kprog_kstar_body puts into a fresh K* — and
// 0 for q >= n and for candidates >= M, as there.  Grid = candidate tiles, workgroup and LDS from kprog_block, every thread walks its
// (row, candidate) entries in a stride loop.  track_append_kernel<true> (grad_kernels.hpp) reads the buffer where the built-in
// instantiation evaluates kappa_r2: the interpreter's LDS column per thread does not fit beside that kernel's 256 threads
// (96 slots × 256 threads × 8 B > a CU's 160 KiB), so the pair is two launches.
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_track_rhs_kernel(FitProg g, const double* __restrict__ Xsc, int d, int Np, int N0, int n,
                                                                               const double* __restrict__ Csc, int Mp, int M, double amp2,
                                                                               double* __restrict__ rhs) {
    constexpr int BN = 32;
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    const int st = blockDim.x, c0 = blockIdx.x * BN;
    double* out = rhs + (size_t)blockIdx.x * TRACK_ROWS * BN;
    for (int e = threadIdx.x; e < TRACK_ROWS * BN; e += st) {
        const int q = e / BN, c = e % BN;
        out[e] = (q < n && c0 + c < M) ? amp2 * kprog_pair(g, d, Xsc, Np, N0 + q, Csc, Mp, c0 + c, col, st) : 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// Gradients of a program-kernel posterior (boss_kgp_set_grad): the reverse sweep kern_grad behind fit_eval gives all 2d partials
// f_u = ∂f/∂u, f_v = ∂f/∂v of a pair.  A column then holds 2·(2d + nI) doubles, values | adjoints (kprog_grad_slots): the longest
// program takes 96 KiB for one wave, so both kernels opt in to the larger dynamic LDS (KPROG_GRAD_MAX_LDS, within a CU's 160 KiB).
// ------------------------------------------------------------------------------------------
// f(a, b) as kprog_pair, then the sweep: ay[0..d) = f_u, ay[d..2d) = f_v in the column's adjoint slots
__device__ __forceinline__ double kprog_pair_grad(const FitProg& g, int d, const double* __restrict__ A, int lda, int ia,
                                                  const double* __restrict__ B, int ldb, int ib, double* __restrict__ col, int st) {
    const double f = kprog_pair(g, d, A, lda, ia, B, ldb, ib, col, st);
    double* v = col + (size_t)2 * d * st;
    double* ay = v + (size_t)g.nI * st;
    kern_grad(g, col, v, ay, ay + (size_t)2 * d * st, st);
    return f;
}

// Likelihood gradient: the Σ-vector of llgrad_tile_kernel per 64×64 tile of the lower triangle, out[tile][0..d-1] = S_m,
// out[tile][d] = Σ_i K⁻¹_ii, out[tile][d+1] = Σ_i a_i² (diagonal tiles), with G = a aᵀ − K⁻¹ and the stored entry (i, j), i > j, being
// f(u_j, u_i):
//     S_m = Σ_{i>j} G_ij α² D_m(j, i) + ½ Σ_i G_ii α² D_m(i, i) ,   D_m(a, b) = f_u,m u_a,m + f_v,m u_b,m
// (K = α² F + σ² I for any F: llgrad_reduce_kernel and llgrad_finalize follow unchanged, ∂ℓ/∂λ_m = −S_m/(λ_m+1e-8)).  The diagonal term
// is real: a dot-product kernel's k(x, x) depends on λ.  D_m is evaluated as (f_u,m + f_v,m) u_b,m + f_u,m (u_a,m − u_b,m): for a
// stationary kernel the first term is rounding noise and the second the difference form grad_accum_body's comment argues for.
// A thread keeps its row i (its lane) and walks the tile's columns; sums: per thread in ascending column, butterfly over the wave,
// waves in ascending order — no atomics, repeated calls agree bit for bit.
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_llgrad_tile_kernel(FitProg g, const double* __restrict__ Xsc, int d, int N, int Np,
                                                                                 const double* __restrict__ hyp,
                                                                                 const double* __restrict__ Kinv, int ldk,
                                                                                 const double* __restrict__ apart, int nch,
                                                                                 double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* col = reinterpret_cast<double*>(kprog_lds_raw) + threadIdx.x;
    __shared__ double aj[64];
    __shared__ double red[KPROG_MAX_WAVES];
    const int st = blockDim.x, tid = threadIdx.x, t = blockIdx.x, lane = tid & 63, wave = tid >> 6, nw = st >> 6;
    int bi = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
    while (bi * (bi + 1) / 2 > t) --bi;
    const int bj = t - bi * (bi + 1) / 2;
    const double amp2 = hyp[0];
    if (tid < 64) {
        double s = 0.0;
        for (int c = 0; c < nch; ++c) s += apart[(size_t)c * Np + bj * 64 + tid];
        aj[tid] = s;
    }
    const int i = bi * 64 + lane;
    double ai = 0.0;
    for (int c = 0; c < nch; ++c) ai += apart[(size_t)c * Np + i];
    __syncthreads();
    const double* fu = col + (size_t)(2 * d + g.nI) * st;     // the adjoint slots of this column: f_u[d] | f_v[d]
    const double* fv = fu + (size_t)d * st;
    double S[KPROG_MAX_D];
#pragma unroll
    for (int m = 0; m < KPROG_MAX_D; ++m) S[m] = 0.0;
    double tr = 0.0, aa = 0.0;
    for (int jl = wave; jl < 64; jl += nw) {
        const int j = bj * 64 + jl;
        if (i >= N || j >= N || i < j) continue;
        const double kinv = Kinv[(size_t)j * ldk + i];
        (void)kprog_pair_grad(g, d, Xsc, Np, j, Xsc, Np, i, col, st);   // a = j, b = i
        double q = amp2 * (ai * aj[jl] - kinv);
        if (i == j) {
            tr += kinv;
            aa += ai * ai;
            q *= 0.5;
        }
#pragma unroll
        for (int m = 0; m < KPROG_MAX_D; ++m)
            if (m < d) {
                const double ua = col[(size_t)m * st], ub = col[(size_t)(d + m) * st], pu = fu[(size_t)m * st], pv = fv[(size_t)m * st];
                S[m] = __builtin_fma(q, __builtin_fma(pu + pv, ub, pu * (ua - ub)), S[m]);
            }
    }
    for (int m = 0; m < d + 2; ++m) {
        double v = 0.0;
#pragma unroll
        for (int mm = 0; mm < KPROG_MAX_D; ++mm)
            if (mm == m) v = S[mm];
        if (m >= d) v = (m == d) ? tr : aa;
        v = wave_sum(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < nw; ++w) s += red[w];
            out[(size_t)t * (d + 2) + m] = s;
        }
    }
}

// ∇μ, ∇σ² from the W slabs (the place grad_accum_kernel takes for the built-in kernels; same grid, same part layout, so
// grad_finalize_kernel finishes a split tile).  Per candidate j and dimension m, 1/λ_m short for 1/(λ_m+1e-8):
//     ∇μ_m  = ∇m_m + (1/λ_m) Σ_i a_i α² f_v,m(u_i, u*_j)
//     ∇σ²_m = (1/λ_m) α² (f_u,m + f_v,m)(u*_j, u*_j) − (2/λ_m) Σ_i w_ij α² f_v,m(u_i, u*_j)
// The sums T1 = Σ a_i α² f_v,m and T2 = Σ w_ij α² f_v,m go to the slots grad_accum_body uses; the prior variance's own gradient rides
// in T2 as −½ α² (f_u,m + f_v,m)(u*_j, u*_j), added once per candidate (row split 0, row subset 0) — exactly 0 for a stationary kernel.
// Lanes run along the tile's 32 candidates, blockDim.x / 32 row subsets; the sums of the subsets are added in ascending order.
__global__ __launch_bounds__(64 * KPROG_MAX_WAVES) void kprog_grad_accum_kernel(FitProg g, const double* __restrict__ Wslabs,
                                                                                const double* __restrict__ avec, int Np, int N,
                                                                                const double* __restrict__ Xsc, const double* __restrict__ Csc,
                                                                                int d, int Mp, int M, double amp2,
                                                                                const double* __restrict__ invlam,
                                                                                const unsigned char* __restrict__ discrete,
                                                                                const double* __restrict__ mean_grad, double* __restrict__ dmu,
                                                                                double* __restrict__ dvar, double* __restrict__ part) {
    constexpr int BN = 32, NS = 2 * (GRAD_MAX_D + 1);
    extern __shared__ __attribute__((aligned(16))) char kprog_lds_raw[];
    double* lds = reinterpret_cast<double*>(kprog_lds_raw);
    double* col = lds + threadIdx.x;
    const int st = blockDim.x, tid = threadIdx.x, c = tid & 31, rs = tid >> 5, nrs = st >> 5;
    const int bx = blockIdx.x, by = blockIdx.y, ny = gridDim.y;
    const double* W = Wslabs + (size_t)bx * Np * BN;
    const int j = bx * BN + c;                               // (candidates >= M are padding inside Mp: evaluated, never written)
    const double* fu = col + (size_t)(2 * d + g.nI) * st;
    const double* fv = fu + (size_t)d * st;
    double T1[GRAD_MAX_D], T2[GRAD_MAX_D];
#pragma unroll
    for (int m = 0; m < GRAD_MAX_D; ++m) T1[m] = T2[m] = 0.0;
    if (by == 0 && rs == 0) {
        (void)kprog_pair_grad(g, d, Csc, Mp, j, Csc, Mp, j, col, st);
#pragma unroll
        for (int m = 0; m < GRAD_MAX_D; ++m)
            if (m < d) T2[m] = -0.5 * amp2 * (fu[(size_t)m * st] + fv[(size_t)m * st]);
    }
    const int nchunk = (N + GRAD_CHUNK - 1) / GRAD_CHUNK;
    const int cpb = (nchunk + ny - 1) / ny;
    const int rbeg = by * cpb * GRAD_CHUNK;
    const int rend = (rbeg + cpb * GRAD_CHUNK < N) ? rbeg + cpb * GRAD_CHUNK : N;
    for (int r = rbeg + rs; r < rend; r += nrs) {
        const double qa = amp2 * avec[r], qw = amp2 * W[(size_t)r * BN + c];
        (void)kprog_pair_grad(g, d, Xsc, Np, r, Csc, Mp, j, col, st);
#pragma unroll
        for (int m = 0; m < GRAD_MAX_D; ++m)
            if (m < d) {
                const double p = fv[(size_t)m * st];
                T1[m] = __builtin_fma(qa, p, T1[m]);
                T2[m] = __builtin_fma(qw, p, T2[m]);
            }
    }
    __syncthreads();                                         // the columns are done: their LDS becomes red[nrs][NS][BN]
    double* rd = lds + (size_t)rs * NS * BN;
    rd[0 * BN + c] = 0.0;                                    // (slots 0, 1 of the layout are not used)
    rd[1 * BN + c] = 0.0;
#pragma unroll
    for (int m = 0; m < GRAD_MAX_D; ++m) {
        rd[(2 + 2 * m) * BN + c] = T1[m];
        rd[(3 + 2 * m) * BN + c] = T2[m];
    }
    __syncthreads();
    if (ny > 1) {
        // this workgroup's sums (over its row subsets) go to global; grad_finalize_kernel finishes
        double* pw = part + ((size_t)bx * ny + by) * NS * BN;
        for (int slot = rs; slot < NS; slot += nrs) {
            double v = 0.0;
            for (int k = 0; k < nrs; ++k) v += lds[((size_t)k * NS + slot) * BN + c];
            pw[slot * BN + c] = v;
        }
        return;
    }
    if (rs == 0 && j < M) {
        for (int m = 0; m < d; ++m) {
            double t1 = 0.0, t2 = 0.0;
            for (int k = 0; k < nrs; ++k) {
                const double* rk = lds + (size_t)k * NS * BN;
                t1 += rk[(2 + 2 * m) * BN + c];
                t2 += rk[(3 + 2 * m) * BN + c];
            }
            const double il = invlam[m];
            const bool disc = discrete && discrete[m];
            dmu[(size_t)j * d + m] = (disc ? 0.0 : t1 * il) + (mean_grad ? mean_grad[(size_t)j * d + m] : 0.0);
            dvar[(size_t)j * d + m] = disc ? 0.0 : -2.0 * t2 * il;
        }
    }
}
#endif  // __HIPCC__

}  // namespace boss
