// cov_kernels.hpp — full posterior covariance Σ = K** − VᵀV (+ jitter) on the fp64 MFMA, for the gradient-observation and
// nonstationary posteriors (boss_ggp_predict_cov / boss_ngp_predict_cov).  V = L⁻¹K* is what the prediction left in its slab
// scratch: V(n, j) = Vs[(j/BN · Np + n) · BN + j % BN].
//
//   cov_syrk_partial_kernel   one workgroup per (64×64 lower-triangle block pair, chunk of the n range): the block's VᵀV over
//                             that chunk, stored to its own partial slab (no float atomics: bitwise reproducible)
//   cov_finish_kernel<FORM>   the partials summed in chunk order, K** of the form added, Σ(i,j) and Σ(j,i) written from the same
//                             value (exactly symmetric); the Gibbs form clips the diagonal as _clip_var does
#pragma once
#include "acq_kernels.hpp"

namespace boss {

constexpr int COV_T = 64;                                  // output block edge: 2×2 sub-tiles of 32, one per wave
constexpr int COV_FORM_VALUE = 0, COV_FORM_GIBBS = 1;

// block pair index p -> (I, J), I >= J, p = I(I+1)/2 + J
__device__ __forceinline__ void cov_pair(int p, int& I, int& J) {
    int i = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= p) ++i;
    while (i * (i + 1) / 2 > p) --i;
    I = i;
    J = p - i * (i + 1) / 2;
}

// grid (P block pairs, C chunks), 256 threads.  Wave w owns the 32×32 sub-tile (w>>1, w&1) of block pair (I, J): rows are the
// 32 candidates 64I + 32(w>>1) .., columns 64J + 32(w&1) ..; each sub-tile's slab slice is an "NT" operand of GemmDirect with
// lda = BN and the training row n as the contraction index.  Rows n of chunk c: [c·rows, min(Np, (c+1)·rows)), rows a
// multiple of 256.  part[(c·P + p)·4096 + r + 64·s] = Σ_n V(n, 64I + r) V(n, 64J + s) over the chunk (column-major block).
__global__ __launch_bounds__(256) void cov_syrk_partial_kernel(const double* __restrict__ Vs, int Np, int BN, int M, int rows,
                                                               double* __restrict__ part) {
    typedef GemmDirect<1, 1, 2, 2, 8> G1;                  // 32×32 per wave; its row offset is wave·32: undone below
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int p = blockIdx.x, c = blockIdx.y, P = gridDim.x;
    int I, J;
    cov_pair(p, I, J);
    const int a = wave >> 1, b = wave & 1;
    if (I == J && a < b) return;                           // strictly upper sub-tile of a diagonal block: never read
    const int ta = 2 * I + a, tb = 2 * J + b;              // 32-candidate tiles
    if (ta * 32 >= M || tb * 32 >= M) return;              // past the last candidate: never read
    const int n0 = c * rows, K = min(rows, Np - n0);
    const double* A = Vs + ((size_t)(ta * 32 / BN) * Np + n0) * BN + (ta * 32) % BN;
    const double* B = Vs + ((size_t)(tb * 32 / BN) * Np + n0) * BN + (tb * 32) % BN;
    v4d acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = v4d{0.0, 0.0, 0.0, 0.0};
    G1::template run<1, true>(A - 32 * wave, BN, B, BN, K, acc);   // (K a multiple of 256: exact ring tail)
    double* out = part + ((size_t)c * P + p) * (COV_T * COV_T) + 32 * a + (size_t)(32 * b) * COV_T;
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = G1::row_of(0, 0, lane), col = G1::col_of(0, n, i, lane);   // tiles m = 0, 1: rows row, row + 1
            *reinterpret_cast<v2d*>(out + row + (size_t)col * COV_T) = v2d{acc[0][n][i], acc[1][n][i]};
        }
}

// grid P, 256 threads: block pair (I, J) of Σ.  FORM_VALUE: K** = amp2 κ(r²) on the scaled candidates X (ldx = Mp), no jitter,
// no clipping (gradient_gp.jl:368-373).  FORM_GIBBS: K** = Gibbs kernel on the rounded raw candidates X with λ(x*) = Lam and
// α(x*) = Amp, + 1e-18 on the diagonal, diagonal through _clip_var (gaussian_process.jl:163-167,180-184): the first index below
// −1e-8 goes to bad (integer atomicMin), values from −1e-8 up to 0 become 0.
template <int FORM>
__global__ __launch_bounds__(256) void cov_finish_kernel(const double* __restrict__ part, int C, const double* __restrict__ X,
                                                         const double* __restrict__ Lam, const double* __restrict__ Amp, int d,
                                                         int ldx, int kern, double amp2, int M, double* __restrict__ cov,
                                                         unsigned long long* __restrict__ bad) {
    __shared__ double T[COV_T][COV_T + 1];                 // T[r][s] = Σ(64I + r, 64J + s)
    const int p = blockIdx.x, P = gridDim.x, tid = threadIdx.x;
    int I, J;
    cov_pair(p, I, J);
    const int i0 = I * COV_T, j0 = J * COV_T;
#pragma unroll 4
    for (int e = tid; e < COV_T * COV_T; e += 256) {
        const int r = e & (COV_T - 1), s = e >> 6;
        const int i = i0 + r, j = j0 + s;
        if (i >= M || j >= M || (I == J && r < s)) continue;
        double acc = 0.0;
        for (int c = 0; c < C; ++c) acc += part[((size_t)c * P + p) * (COV_T * COV_T) + e];
        double kss;
        if constexpr (FORM == COV_FORM_VALUE) {
            double r2 = 0.0;
            for (int k = 0; k < d; ++k) {
                const double df = X[(size_t)k * ldx + i] - X[(size_t)k * ldx + j];
                r2 = __builtin_fma(df, df, r2);
            }
            kss = amp2 * kappa_r2(kern, r2);
        } else {
            double pr = 1.0, es = 0.0;
            for (int k = 0; k < d; ++k)
                gibbs_dim(X[(size_t)k * ldx + i], Lam[(size_t)k * ldx + i], X[(size_t)k * ldx + j], Lam[(size_t)k * ldx + j], pr, es);
            const double am = 0.5 * (Amp[i] + Amp[j]);
            kss = am * am * sqrt(pr) * exp(-es);
        }
        double v = kss - acc;
        if constexpr (FORM == COV_FORM_GIBBS) {
            if (i == j) {
                v += PREDICT_JITTER;
                if (v < 0.0) {
                    if (v >= -MAX_NEG_VAR) v = 0.0;
                    else atomicMin(bad, (unsigned long long)i);
                }
            }
        }
        T[r][s] = v;
    }
    __syncthreads();
    // block (I, J), column-major, lanes along the rows; the strictly upper part of a diagonal block mirrors its lower part
    for (int e = tid; e < COV_T * COV_T; e += 256) {
        const int r = e & (COV_T - 1), s = e >> 6;
        if (i0 + r < M && j0 + s < M) cov[(size_t)(j0 + s) * M + i0 + r] = (I == J && r < s) ? T[s][r] : T[r][s];
    }
    if (I == J) return;
    // the mirrored block (J, I): Σ(64J + r, 64I + s) = T[s][r]
    for (int e = tid; e < COV_T * COV_T; e += 256) {
        const int r = e & (COV_T - 1), s = e >> 6;
        if (j0 + r < M && i0 + s < M) cov[(size_t)(i0 + s) * M + j0 + r] = T[s][r];
    }
}

}  // namespace boss
