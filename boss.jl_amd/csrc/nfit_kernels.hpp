// nfit_kernels.hpp — the nonstationary likelihood in the WHITENED parameters of its latent ParametrizedGPs (boss_nfit_*).
//
// A fitter of the reference moves yϵ of every latent (parametrized_gp.jl:49-77); the latent's values at the data are
//     v = act(target(L yϵ + μ))                       (parametrized_gp.jl:108-120, the closed forms of nlat_transform)
// and the gradient of the data term comes back as  Lᵀ (c ⊙ v′)  with c the cotangents of boss_ngp_loglike_grad.  Per chunk of sets:
//   nfit_tri_gemm_kernel<false>   Y_f = L_f Θ_f        lower-triangular × dense on the fp64 MFMA tile core (GemmNT), per factor,
//                                                      all columns (latents sharing f × sets); k-tiles above the diagonal are skipped
//   nfit_transform_kernel         v, v′ of every latent at every point: v into the sets' parameter blocks (the very layout
//                                 ngp_stage_set uploads: λ [d][Np] | α [Np] | σ [Np], padding λ = 1, α = σ = 0), v′ over Y in place;
//                                 an invalid value (or a NaN) raises the set's integer flag; scalar latents broadcast
//   nfit_neutralise_kernel        flagged sets get the all-ones block ngp_stage_set gives an invalid set
//   (Gram, factorisation, gradient pass of the batched likelihood)
//   nfit_cotangent_kernel         W = C ⊙ V′ in the [point][column] layout the tile core wants; fixed-order sums for scalar latents
//   nfit_tri_gemm_kernel<true>    G_f = L_fᵀ W_f        the same core on a resident transposed copy of the factor (upper triangular:
//                                                      the k-tiles LEFT of the diagonal are skipped)
// The contraction runs over ascending k in every tile, whatever tile column a column sits in, and one MFMA output depends on its own
// B column only: a set's numbers do not depend on the batch around it.  No floating-point atomics.
// Operand layouts (GemmNT: contraction index = column index of both operands): the factor column-major with leading dimension
// Nk = N rounded up to 64, zero beyond N; Θ and W as B[col + k·ldb], i.e. one ROW per point, padded columns zero.  Results are
// column-major [col][Nk].
#pragma once
#include "gemm_f64.hpp"
#include "latent_kernels.hpp"

namespace boss {

typedef GemmNT<4, 1, 1, 2> NfitG;           // 64 rows × 32 columns per workgroup: many workgroups at a handful of columns
constexpr int NFIT_BM = NfitG::BM, NFIT_BN = NfitG::BN;

struct NfitLatent {                         // one latent of the output
    const double* mu;                       // [N] or null = zeros (GP latents)
    int gp;                                 // 1: whitened GP latent, 0: scalar
    int col0, nf;                           // GP: column of set b is col0 + b·nf   (nf latents share the factor)
    int target, act;
    double tp0, tp1, ap;
};
struct NfitDesc {                           // the d + 2 latents of the output, passed to the kernels by value (the columns depend on the chunk)
    NfitLatent lat[NLAT_MAX_D + 2];
};

// C[col][Nk] = A · B over the k-tiles in which the triangular A is non-zero.  grid = (Nk / 64, columns / 32).
// UPPER = false: A lower triangular, k in [0, 64 (rt + 1));  UPPER = true: A upper triangular, k in [64 rt, Nk).
template <bool UPPER>
__global__ __launch_bounds__(256) void nfit_tri_gemm_kernel(const double* __restrict__ A, int Nk, const double* __restrict__ B, int ldb,
                                                            int col0, double* __restrict__ Cout) {
    __shared__ double lds[NfitG::LDS_DOUBLES];
    const int rt = blockIdx.x, c0 = col0 + blockIdx.y * NFIT_BN;
    const int k0 = UPPER ? rt * NFIT_BM : 0, K = UPPER ? Nk - k0 : (rt + 1) * NFIT_BM;
    v4d acc[NfitG::TM][NfitG::TN];
#pragma unroll
    for (int m = 0; m < NfitG::TM; ++m)
#pragma unroll
        for (int n = 0; n < NfitG::TN; ++n) acc[m][n] = v4d{0.0, 0.0, 0.0, 0.0};
    NfitG::run(A + (size_t)rt * NFIT_BM + (size_t)k0 * Nk, Nk, B + c0 + (size_t)k0 * ldb, ldb, K, acc, lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave / NfitG::WC, wc = wave % NfitG::WC;
#pragma unroll
    for (int m = 0; m < NfitG::TM; ++m)
#pragma unroll
        for (int n = 0; n < NfitG::TN; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = rt * NFIT_BM + NfitG::row_of(wr, m, lane), col = c0 + NfitG::col_of(wc, n, i, lane);
                Cout[(size_t)col * Nk + row] = acc[m][n][i];
            }
}

// grid = (Np / 256, d + 2, sets from b0).  Y [col][Nk]: in L yϵ, out v′.  scal [set][d + 2]: the scalar latents' values.
__global__ __launch_bounds__(256) void nfit_transform_kernel(const NfitDesc D, int d, int N, int Np, int Nk,
                                                             double* __restrict__ Y, const double* __restrict__ scal,
                                                             double* __restrict__ par, size_t par_doubles, int* __restrict__ flags, int b0) {
    const int j = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, b = b0 + blockIdx.z;
    if (j >= Np) return;
    double* p = par + (size_t)b * par_doubles + (size_t)q * Np;
    if (j >= N) {
        p[j] = q < d ? 1.0 : 0.0;
        return;
    }
    const NfitLatent L = D.lat[q];
    double v, m = 0.0;
    if (L.gp) {
        double* yp = Y + (size_t)(L.col0 + b * L.nf) * Nk + j;
        m = *yp + (L.mu ? L.mu[j] : 0.0);
        NlatLatent T;
        T.target = L.target;
        T.act = L.act;
        T.tp0 = L.tp0;
        T.tp1 = L.tp1;
        T.ap = L.ap;
        double dv;
        nlat_transform(T, m, v, dv);
        *yp = dv;
    } else {
        v = scal[(size_t)b * (d + 2) + q];
    }
    const bool ok = m == m && (q < d ? (v > 0.0 && isfinite(v)) : (v >= 0.0 && isfinite(v)));
    if (!ok) atomicOr(flags + b, 1);
    p[j] = v;
}

// grid = (Np / 256, d + 2, sets): the block of a flagged set as ngp_stage_set stages an invalid set
__global__ __launch_bounds__(256) void nfit_neutralise_kernel(int N, int Np, double* __restrict__ par, size_t par_doubles,
                                                              const int* __restrict__ flags, int b0) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = b0 + blockIdx.z;
    if (j < N && flags[b]) par[(size_t)b * par_doubles + (size_t)blockIdx.y * Np + j] = 1.0;
}

// grid = (Nk / 256 rounded up, d + 2, sets).  cot: the sets' cotangents, row q of set b at cot + b·cot_doubles + q·Np.
// GP latent: W[j][col] = c_j v′_j (zero for j in [N, Nk)).  Scalar latent (workgroup x = 0 only): Σ_j c_j in a fixed order.
__global__ __launch_bounds__(256) void nfit_cotangent_kernel(const NfitDesc D, int d, int N, int Np, int Nk,
                                                             const double* __restrict__ cot, size_t cot_doubles,
                                                             const double* __restrict__ V, double* __restrict__ W, int ldw,
                                                             double* __restrict__ sg, int b0) {
    __shared__ double red[256];
    const int q = blockIdx.y, b = b0 + blockIdx.z, tid = threadIdx.x;
    const NfitLatent L = D.lat[q];
    const double* c = cot + (size_t)b * cot_doubles + (size_t)q * Np;
    if (L.gp) {
        const int j = blockIdx.x * 256 + tid;
        if (j >= Nk) return;
        const int col = L.col0 + b * L.nf;
        W[(size_t)j * ldw + col] = j < N ? c[j] * V[(size_t)col * Nk + j] : 0.0;
        return;
    }
    if (blockIdx.x != 0) return;
    double s = 0.0;
    for (int j = tid; j < N; j += 256) s += c[j];
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) sg[(size_t)b * (d + 2) + q] = red[0];
}

}  // namespace boss
