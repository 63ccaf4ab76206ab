// prune_kernels.hpp — arg-max-only acquisition: an upper bound on every candidate's EI from the exact mean and the variance
// after the first s 256-row blocks of the substitution, the selection of the contenders, and the merge of their exact values
// (host side: host_prune.inc).
#pragma once
#include "acq_kernels.hpp"

namespace boss {

// ------------------------------------------------------------------------------------------
// a = L⁻ᵀ z read from L's own columns (no transposed factor), one launch per 256-row step from the last block to the first:
//     a_i = Dinv2_iᵀ r_i                     every workgroup forms it from the finished residual (LDS); workgroup 0 stores it
//     r_j −= L_ijᵀ a_i   for j < i           128 columns of L per workgroup, eight per wave, lanes along the contiguous rows
// r starts as z (read from row Np of the factor array by the first step, zero behind row N).  Every sum has a fixed order.
// ------------------------------------------------------------------------------------------
// v[j] = this lane's share of sum j (NC sums, NC a power of two <= 64): afterwards v[0] of lane l is the whole sum number l % NC over
// the wave.  Halving exchange: each step sends the half a lane does not keep to its partner, so 64 sums cost 63 shuffles, not 384;
// the order of the additions is fixed by the lane numbers.
template <int NC>
__device__ __forceinline__ void prune_wave_sums(double (&v)[NC], int lane) {
#pragma unroll
    for (int h = NC / 2; h >= 1; h >>= 1) {
        const bool up = (lane & h) != 0;
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const double keep = up ? v[j + h] : v[j], send = up ? v[j] : v[j + h];
            v[j] = keep + __shfl_xor(send, h);
        }
    }
#pragma unroll
    for (int off = NC; off < 64; off <<= 1) v[0] += __shfl_xor(v[0], off);
}
constexpr int PRUNE_AVEC_THREADS = 1024;                     // 16 waves: the loads of a step are all in flight at once
__global__ __launch_bounds__(PRUNE_AVEC_THREADS) void prune_avec_step_kernel(const double* __restrict__ A, int ld, int Np, int N,
                                                                             const double* __restrict__ Dinv2, int ib, int first,
                                                                             double* __restrict__ r, double* __restrict__ a) {
    __shared__ double rv[PRED_RB], av[PRED_RB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i0 = ib * PRED_RB;
    if (tid < PRED_RB) {
        const int i = i0 + tid;
        rv[tid] = first ? (i < N ? A[(size_t)i * ld + Np] : 0.0) : r[i];
    }
    __syncthreads();
    const double* D = Dinv2 + (size_t)ib * PRED_RB * PRED_RB;   // column-major, lower triangular (what lies above the diagonal is not used)
    double r4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) r4[q] = rv[lane + 64 * q];
    {
        // wave w takes the columns 16 j + w (equal shares of the triangle); a column needs the 64-row chunks from its own on
        double sums[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = 16 * j + wave;
            const double* col = D + (size_t)c * PRED_RB;
            double sacc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (q >= j / 4) {                             // (compile-time: chunk q holds rows >= c only from c / 64 on)
                    const int row = lane + 64 * q;
                    const double dv = col[row];
                    sacc = __builtin_fma(row >= c ? dv : 0.0, r4[q], sacc);
                }
            }
            sums[j] = sacc;
        }
        prune_wave_sums<16>(sums, lane);
        if (lane < 16) av[16 * lane + wave] = sums[0];
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid < PRED_RB) a[i0 + tid] = av[tid];
    if (ib == 0) return;
    double a4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) a4[q] = av[lane + 64 * q];
    double sums[8];
    const int cg0 = blockIdx.x * 128 + wave * 8;             // columns of L before block ib (grid = 2·ib workgroups)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double* col = A + (size_t)(cg0 + j) * ld + i0;
        double sacc = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) sacc = __builtin_fma(col[lane + 64 * q], a4[q], sacc);
        sums[j] = sacc;
    }
    prune_wave_sums<8>(sums, lane);
    if (lane < 8) {
        const int cg = cg0 + lane;
        const double base = first ? (cg < N ? A[(size_t)cg * ld + Np] : 0.0) : r[cg];
        r[cg] = base - sums[0];
    }
}

// ------------------------------------------------------------------------------------------
// Head variance σ²_s = α² − Σ_{rows < 256·s} v² + jitter: predict_body's arithmetic (predict_kernels.hpp) over the first sblk row
// blocks only — the posterior variance given the first 256·s observations, an upper bound on the final one.  The V slab of a
// workgroup has sblk·256 rows; Xsc keeps Np as its leading dimension.
// ------------------------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(G::NTHREADS) __attribute__((amdgpu_waves_per_eu(1, 1))) void prune_head_kernel(
    const double* __restrict__ A, int ld, int Np, int N, const double* __restrict__ Dinv, const double* __restrict__ Xsc,
    const double* __restrict__ Csc, int d, int Mp, int kern, double amp2, double* __restrict__ Vscratch, int M, int sblk,
    double* __restrict__ var_out) {
    static_assert(G::WC == 1 && G::BM == 2 * BLK && G::PM == 2 && G::WR == 4, "written for the 256-row, 32-candidate geometry");
    constexpr int RB = G::BM;
    extern __shared__ double lds[];
    constexpr int BN = G::BN, TM = G::TM, TN = G::TN, LDR = PredictLds<G>::LDR;
    double* Rs = lds;
    double* red = Rs + RB * LDR;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave, wc = 0;
    const int tile = blockIdx.x, c0 = tile * BN;
    double* V = Vscratch + (size_t)tile * sblk * RB * BN;
    double* part = red + 2 * G::WR * G::BN;
#pragma unroll
    for (int u = 0; u < TN * 4; ++u) part[u * G::NTHREADS + tid] = 0.0;
    double* cs = part + (size_t)G::NTHREADS * PredictLds<G>::PART;
    const bool cs_ok = d <= PRED_CS_MAX_D;
    if (cs_ok) {
        for (int idx = tid; idx < d * BN; idx += G::NTHREADS) cs[idx] = Csc[(size_t)(idx / BN) * Mp + c0 + (idx % BN)];
        __syncthreads();
    }
    for (int ib = 0; ib < sblk; ++ib) {
        v4d acc[TM][TN];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int n = 0; n < TN; ++n) acc[m][n] = v4d{0.0, 0.0, 0.0, 0.0};
        G::template run<1>(A + (size_t)ib * RB, ld, V, BN, ib * RB, acc);
        double r2[TM][TN][4];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int n = 0; n < TN; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) r2[m][n][i] = 0.0;
        if (cs_ok) {
            for (int kd0 = 0; kd0 < d; kd0 += 4) {
                double xr[4][TM];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int m = 0; m < TM; ++m)
                        xr[kk][m] = (kd0 + kk < d) ? Xsc[(size_t)(kd0 + kk) * Np + ib * RB + G::row_of(wr, m, lane)] : 0.0;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    if (kd0 + kk < d) {
#pragma unroll
                        for (int n = 0; n < TN; ++n)
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const double xc = cs[(kd0 + kk) * BN + G::col_of(wc, n, i, lane)];
#pragma unroll
                                for (int m = 0; m < TM; ++m) {
                                    const double diff = xr[kk][m] - xc;
                                    r2[m][n][i] = __builtin_fma(diff, diff, r2[m][n][i]);
                                }
                            }
                    }
                }
            }
        } else
        for (int kd = 0; kd < d; ++kd) {
            double xr[TM], xc[TN][4];
#pragma unroll
            for (int m = 0; m < TM; ++m) xr[m] = Xsc[(size_t)kd * Np + ib * RB + G::row_of(wr, m, lane)];
#pragma unroll
            for (int n = 0; n < TN; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) xc[n][i] = Csc[(size_t)kd * Mp + c0 + G::col_of(wc, n, i, lane)];
#pragma unroll
            for (int m = 0; m < TM; ++m)
#pragma unroll
                for (int n = 0; n < TN; ++n)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        double diff = xr[m] - xc[n][i];
                        r2[m][n][i] = __builtin_fma(diff, diff, r2[m][n][i]);
                    }
        }
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            const int row = G::row_of(wr, m, lane);
            const bool live = (ib * RB + row) < N;
#pragma unroll
            for (int n = 0; n < TN; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double ks = live ? amp2 * kappa_r2(kern, r2[m][n][i]) : 0.0;
                    Rs[row * LDR + G::col_of(wc, n, i, lane)] = ks - acc[m][n][i];
                }
        }
        __syncthreads();                                   // R tile complete
        v4d acc2[TM][TN];
#pragma unroll
        for (int m = 0; m < TM; ++m)
#pragma unroll
            for (int n = 0; n < TN; ++n) acc2[m][n] = v4d{0.0, 0.0, 0.0, 0.0};
        G::run_Blds_tri(Dinv + (size_t)ib * RB * RB, RB, Rs, LDR, acc2);
#pragma unroll
        for (int m = 0; m < TM; ++m) {
            const int row = ib * RB + G::tri_row_of(wr, m, lane);
#pragma unroll
            for (int n = 0; n < TN; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double v = acc2[m][n][i];
                    if (ib + 1 < sblk) V[(size_t)row * BN + G::col_of(wc, n, i, lane)] = v;   // (the last block's V has no reader)
                    double* ps = part + (size_t)(n * 4 + i) * G::NTHREADS + tid;
                    ps[0] = __builtin_fma(v, v, ps[0]);
                }
        }
        __syncthreads();                                   // V_ib visible to the whole workgroup; Rs reusable
    }
#pragma unroll
    for (int n = 0; n < TN; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double s = part[(size_t)(n * 4 + i) * G::NTHREADS + tid];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off);
            if ((lane & 15) == 0) red[wr * BN + G::col_of(wc, n, i, lane)] = s;
        }
    __syncthreads();
    if (tid < BN) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < G::WR; ++w) s += red[w * BN + tid];
        const int j = c0 + tid;
        if (j < M) var_out[j] = amp2 - s + PREDICT_JITTER;
    }
}

// ------------------------------------------------------------------------------------------
// Exact means without the substitution: part[ch][j] = Σ_{n in 128-row chunk ch} α² κ(x_n, c_j) a_n  (grid = 512-candidate groups
// × row chunks; two candidates per thread, rows staged 64 at a time in LDS and taken eight at a time).  K* is not stored.
// REG: x_dim <= 16, the candidate's coordinates stay in registers.
// ------------------------------------------------------------------------------------------
constexpr int PRUNE_MU_STAGE = 64, PRUNE_MU_ROWS = 128, PRUNE_MU_CANDS = 512;
template <bool REG>
__global__ __launch_bounds__(256) void prune_mu_kernel(const double* __restrict__ Xsc, int Np, int N, const double* __restrict__ Csc,
                                                       int d, int Mp, int M, int kern, double amp2, const double* __restrict__ a,
                                                       double* __restrict__ part) {
    extern __shared__ double sm[];                           // [d][64] row coordinates | [64] a
    double* xs = sm;
    double* as = sm + (size_t)d * PRUNE_MU_STAGE;
    const int j0 = blockIdx.x * PRUNE_MU_CANDS + threadIdx.x, j1 = j0 + 256;      // two candidates per thread share every LDS read
    const int jc0 = j0 < Mp ? j0 : Mp - 1, jc1 = j1 < Mp ? j1 : Mp - 1;
    const int rbase = blockIdx.y * PRUNE_MU_ROWS;
    double cx0[REG ? 16 : 1], cx1[REG ? 16 : 1];
    if (REG) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            cx0[k] = k < d ? Csc[(size_t)k * Mp + jc0] : 0.0;
            cx1[k] = k < d ? Csc[(size_t)k * Mp + jc1] : 0.0;
        }
    }
    double acc0 = 0.0, acc1 = 0.0;
    for (int sub = 0; sub < PRUNE_MU_ROWS / PRUNE_MU_STAGE; ++sub) {
        const int r0 = rbase + sub * PRUNE_MU_STAGE;
        __syncthreads();
        for (int idx = threadIdx.x; idx < d * PRUNE_MU_STAGE; idx += 256)
            xs[idx] = Xsc[(size_t)(idx / PRUNE_MU_STAGE) * Np + r0 + (idx % PRUNE_MU_STAGE)];
        if (threadIdx.x < PRUNE_MU_STAGE) as[threadIdx.x] = (r0 + threadIdx.x < N) ? a[r0 + threadIdx.x] : 0.0;
        __syncthreads();
        if (r0 >= N) continue;                               // (uniform: padded rows carry nothing)
        for (int rg = 0; rg < PRUNE_MU_STAGE; rg += 8) {
            double ra[8], rb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) ra[i] = rb[i] = 0.0;
            if (REG) {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < d) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const double x = xs[k * PRUNE_MU_STAGE + rg + i];
                            const double da = x - cx0[k], db = x - cx1[k];
                            ra[i] = __builtin_fma(da, da, ra[i]);
                            rb[i] = __builtin_fma(db, db, rb[i]);
                        }
                    }
            } else {
                for (int k = 0; k < d; ++k) {
                    const double ca = Csc[(size_t)k * Mp + jc0], cb = Csc[(size_t)k * Mp + jc1];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const double x = xs[k * PRUNE_MU_STAGE + rg + i];
                        const double da = x - ca, db = x - cb;
                        ra[i] = __builtin_fma(da, da, ra[i]);
                        rb[i] = __builtin_fma(db, db, rb[i]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double ai = as[rg + i];
                if (r0 + rg + i < N) {
                    acc0 = __builtin_fma(amp2 * kappa_r2(kern, ra[i]), ai, acc0);
                    acc1 = __builtin_fma(amp2 * kappa_r2(kern, rb[i]), ai, acc1);
                }
            }
        }
    }
    if (j0 < M) part[(size_t)blockIdx.y * M + j0] = acc0;
    if (j1 < M) part[(size_t)blockIdx.y * M + j1] = acc1;
}

// ------------------------------------------------------------------------------------------
// Bounds, selection, decision.  Selection and decision are single-workgroup kernels of 1024 threads over the M candidates.
// ------------------------------------------------------------------------------------------
constexpr int PRUNE_THREADS = 1024;
struct PrunePar {
    double coef, best, amp2;
    double kmu, kvar;          // slack factors: δμ = kmu (|c μ| + |best| + |c| α), δv = kvar α²
};
__device__ __forceinline__ double prune_dmu(const PrunePar& pp, double muf) {
    return pp.kmu * (fabs(muf) + fabs(pp.best) + fabs(pp.coef) * sqrt(pp.amp2));
}
// EI(c μ − best + δμ, c² (σ²_s + δv)) by ei_value's formulas; anything not finite comes back NaN (its candidate survives)
__device__ __forceinline__ double prune_bound(const PrunePar& pp, double mu, double var) {
    if (var < 0.0) {
        if (var >= -MAX_NEG_VAR) var = 0.0;
        else return NAN;
    }
    const double muf = pp.coef * mu;
    const double vf = pp.coef * pp.coef * (var + pp.kvar * pp.amp2);
    const double sf = sqrt(vf), diff = muf - pp.best + prune_dmu(pp, muf);
    double ei;
    if (diff == 0.0 && sf == 0.0) ei = 0.0;
    else {
        const double z = diff / sf;
        ei = diff * normcdf_dev(z) + sf * normpdf_dev(z);
    }
    return (ei - ei == 0.0) ? ei : NAN;
}
// order-preserving 64-bit key of a bound; NaN sorts above everything
__device__ __forceinline__ unsigned long long prune_key(double v) {
    if (v != v) return ~0ull;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// exclusive scan of one int per thread over the workgroup (PRUNE_THREADS entries of buf); returns this thread's offset, *total the sum
__device__ __forceinline__ int prune_exscan(int v, int* buf, int* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < PRUNE_THREADS; off <<= 1) {
        const int add = t >= off ? buf[t - off] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const int incl = buf[t];
    *total = buf[PRUNE_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// μ_a = m + Σ_ch part[ch] (chunk order), the bound and its key, one candidate per thread
__global__ __launch_bounds__(256) void prune_bound_kernel(const double* __restrict__ part, int nch, const double* __restrict__ mean_s,
                                                          const double* __restrict__ var_s, const unsigned char* __restrict__ mask, int M,
                                                          PrunePar pp, double* __restrict__ mua, double* __restrict__ ub,
                                                          unsigned long long* __restrict__ keys) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    double m = mean_s ? mean_s[j] : 0.0;
    for (int ch = 0; ch < nch; ++ch) m += part[(size_t)ch * M + j];
    mua[j] = m;
    const double u = (mask && !mask[j]) ? 0.0 : prune_bound(pp, m, var_s[j]);
    ub[j] = u;
    keys[j] = prune_key(u);
}

// one count per active lane into hist[bin], lanes of a wave that share a bin combined into one LDS atomic (the leading bytes of
// the keys are nearly all equal: one atomic per key would serialise the whole pass)
__device__ __forceinline__ void prune_hist_add(int* hist, int bin, bool active, int lane) {
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int b = __shfl(bin, leader);
        const unsigned long long same = __ballot(active && bin == b);
        if (lane == leader) atomicAdd(&hist[b], (int)__popcll(same));
        todo &= ~same;
    }
}

// The K candidates with the largest bounds (radix select over the keys, ties at the K-th key by index): sel[0..K) in ascending
// index order, insel[j] = 1 for them.  Requires K <= M <= PRUNE_THREADS · PRUNE_CPT_MAX (the keys of a thread stay in registers).
constexpr int PRUNE_CPT_MAX = 16;
__global__ __launch_bounds__(PRUNE_THREADS) void prune_select_kernel(const unsigned long long* __restrict__ keys, int M, int K,
                                                                     int* __restrict__ sel, unsigned char* __restrict__ insel) {
    __shared__ int hist[256];
    __shared__ int scan[PRUNE_THREADS];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_remaining;
    const int t = threadIdx.x, lane = t & 63;
    unsigned long long kreg[PRUNE_CPT_MAX];
#pragma unroll
    for (int i = 0; i < PRUNE_CPT_MAX; ++i) {
        const int j = t + PRUNE_THREADS * i;
        kreg[i] = j < M ? keys[j] : 0ull;
    }
    if (t == 0) {
        s_prefix = 0ull;
        s_remaining = K;
    }
    __syncthreads();
    for (int pass = 7; pass >= 0; --pass) {
        if (t < 256) hist[t] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        const int sh = 8 * pass;
#pragma unroll
        for (int i = 0; i < PRUNE_CPT_MAX; ++i) {
            const unsigned long long k = kreg[i];
            const bool in = (t + PRUNE_THREADS * i < M) && (pass == 7 || (k >> (sh + 8)) == (prefix >> (sh + 8)));
            prune_hist_add(hist, (int)((k >> sh) & 255ull), in, lane);
        }
        __syncthreads();
        // suffix sums over the bins (256 threads), then the one bin where they first reach what is still wanted
        const int rem = s_remaining;
        int suf = t < 256 ? hist[t] : 0;
        for (int off = 1; off < 256; off <<= 1) {
            const int add = (t < 256 && t + off < 256) ? hist[t + off] : 0;
            __syncthreads();
            if (t < 256) {
                suf += add;
                hist[t] = suf;
            }
            __syncthreads();
        }
        const int above = (t < 255) ? hist[t + 1] : 0;        // keys in the bins above t
        __syncthreads();
        if (t < 256 && suf >= rem && above < rem) {          // (exactly one t: K <= M keys match the prefix)
            s_remaining = rem - above;                       // of the keys equal to the prefix so far, that many are still wanted
            s_prefix = prefix | ((unsigned long long)t << sh);
        }
        __syncthreads();
    }
    const unsigned long long kth = s_prefix;
    const int want_eq = s_remaining;
    // ordered compaction: thread t owns the contiguous indices [t·cpt, (t+1)·cpt)
    const int cpt = (M + PRUNE_THREADS - 1) / PRUNE_THREADS;
    const int j0 = t * cpt, j1 = min(M, j0 + cpt);
    int ngt = 0, neq = 0;
    for (int j = j0; j < j1; ++j) {
        const unsigned long long k = keys[j];
        ngt += k > kth;
        neq += k == kth;
    }
    int tot_gt, tot_eq;
    const int eq_off = prune_exscan(neq, scan, &tot_eq);
    int take = 0, eqr = eq_off;                              // equals are taken in index order until want_eq are in
    for (int j = j0; j < j1; ++j) {
        const unsigned long long k = keys[j];
        if (k > kth) ++take;
        else if (k == kth) {
            if (eqr < want_eq) ++take;
            ++eqr;
        }
    }
    (void)ngt;
    const int off = prune_exscan(take, scan, &tot_gt);
    int o = off;
    eqr = eq_off;
    for (int j = j0; j < j1; ++j) {
        const unsigned long long k = keys[j];
        bool in = k > kth;
        if (k == kth) {
            in = eqr < want_eq;
            ++eqr;
        }
        insel[j] = in ? 1 : 0;
        if (in) {
            if (o < K) sel[o] = j;
            ++o;
        }
    }
}

// the listed candidates' coordinates (and prior means) into an internal resident block of Mpi columns; columns behind n are zero
__global__ __launch_bounds__(256) void prune_gather_kernel(const int* __restrict__ list, int n, const double* __restrict__ Craw, int Mp,
                                                           int d, const double* __restrict__ mean_s, double* __restrict__ Cint, int Mpi,
                                                           double* __restrict__ mean_int) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Mpi) return;
    const int j = i < n ? list[i] : -1;
    for (int k = 0; k < d; ++k) Cint[(size_t)k * Mpi + i] = j >= 0 ? Craw[(size_t)k * Mp + j] : 0.0;
    if (mean_int) mean_int[i] = (j >= 0 && mean_s) ? mean_s[j] : 0.0;
}

// exact EI of the n listed candidates from their finished moments, the first-index arg-max among them (better()), and the run-time
// check of the mean: *bad is set where |c| |μ_a − μ| exceeds a tenth of the mean slack (with a zero slack: where they differ at all)
__device__ __forceinline__ void prune_exact_reduce(const int* __restrict__ list, int n, const double* __restrict__ imu,
                                                   const double* __restrict__ ivar, const double* __restrict__ mua,
                                                   const unsigned char* __restrict__ mask, const EiPar& par, const PrunePar& pp,
                                                   double* sv, long* si, double& bv, long& bi, int* bad) {
    constexpr long NONE = 0x7fffffffffffffffL;
    const int t = threadIdx.x;
    double v = -INFINITY;
    long ix = NONE;
    for (int i = t; i < n; i += PRUNE_THREADS) {
        const long j = list[i];
        const double m = imu[i];
        double e = ei_value_one(m, ivar[i], par);
        if (mask && !mask[j]) e = 0.0;
        else if (!(fabs(pp.coef) * fabs(mua[j] - m) <= 0.1 * prune_dmu(pp, pp.coef * m)) && m == m) atomicOr(bad, 1);
        if (ix == NONE || better(e, j, v, ix)) {
            v = e;
            ix = j;
        }
    }
    sv[t] = v;
    si[t] = ix;
    __syncthreads();
    for (int st = PRUNE_THREADS / 2; st > 0; st >>= 1) {
        if (t < st) {
            const double ov = sv[t + st];
            const long oi = si[t + st];
            if (oi != NONE && (si[t] == NONE || better(ov, oi, sv[t], si[t]))) {
                sv[t] = ov;
                si[t] = oi;
            }
        }
        __syncthreads();
    }
    bv = sv[0];
    bi = si[0];
    __syncthreads();
}

// Can candidate j, outside round 1, still win against round 1's (T, iT)?  Not with ub_j < T.  With ub_j == T it can at most tie, and
// a tie goes to the lower index: it survives only below iT.  That second rule needs EI_j <= ub_j to the last bit, which holds for a
// masked candidate (both are exactly 0) and wherever T is a normal number; below that the EI formula's products round in
// denormals and a bound can come out a step or two of 4.9e-324 under the exact value (seen: −1e-323), so there the bound is taken
// 64 steps higher and ub_j == T keeps j.  A NaN bound always survives, and a NaN T excludes nothing.
__device__ __forceinline__ bool prune_survives(double u, double T, long iT, long j, bool masked) {
    if (!masked && T < 2.2250738585072014e-308) u += 64 * 4.9406564584124654e-324;
    if (u < T) return false;
    if (u > T || u != u || j < iT) return true;
    return !(masked || T >= 2.2250738585072014e-308);
}

// Round 1 is finished: T = its maximum, survivors = {j outside round 1 : prune_survives} compacted in index order into surv.
// res (mapped host memory): {T, first index, survivor count, mean-check flag}, then the sequence word the host polls.
__global__ __launch_bounds__(PRUNE_THREADS) void prune_decide_kernel(const int* __restrict__ sel, int K, const double* __restrict__ imu,
                                                                     const double* __restrict__ ivar, const double* __restrict__ mua,
                                                                     const unsigned char* __restrict__ mask, EiPar par, PrunePar pp, int M,
                                                                     const double* __restrict__ ub, const unsigned char* __restrict__ insel,
                                                                     int* __restrict__ surv, double* __restrict__ tpair,
                                                                     double* __restrict__ res, unsigned long long res_seq) {
    __shared__ double sv[PRUNE_THREADS];
    __shared__ long si[PRUNE_THREADS];
    __shared__ int scan[PRUNE_THREADS];
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t == 0) bad = 0;
    __syncthreads();
    double T;
    long iT;
    prune_exact_reduce(sel, K, imu, ivar, mua, mask, par, pp, sv, si, T, iT, &bad);
    const int cpt = (M + PRUNE_THREADS - 1) / PRUNE_THREADS;
    const int j0 = t * cpt, j1 = min(M, j0 + cpt);
    int cnt = 0;
    for (int j = j0; j < j1; ++j) cnt += (!insel[j] && prune_survives(ub[j], T, iT, j, mask && !mask[j])) ? 1 : 0;
    int total;
    int o = prune_exscan(cnt, scan, &total);
    for (int j = j0; j < j1; ++j)
        if (!insel[j] && prune_survives(ub[j], T, iT, j, mask && !mask[j])) surv[o++] = j;
    if (t == 0) {
        tpair[0] = T;
        reinterpret_cast<long*>(tpair)[1] = iT;
        res[0] = T;
        reinterpret_cast<long*>(res)[1] = iT;
        reinterpret_cast<long*>(res)[2] = total;
        reinterpret_cast<long*>(res)[3] = bad;
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(res) + 4, res_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Round 2 is finished: the exact values of the n survivors merged with round 1's (T, index) by better()
__global__ __launch_bounds__(PRUNE_THREADS) void prune_merge_kernel(const int* __restrict__ surv, int n, const double* __restrict__ imu,
                                                                    const double* __restrict__ ivar, const double* __restrict__ mua,
                                                                    const unsigned char* __restrict__ mask, EiPar par, PrunePar pp,
                                                                    const double* __restrict__ tpair, double* __restrict__ res,
                                                                    unsigned long long res_seq) {
    __shared__ double sv[PRUNE_THREADS];
    __shared__ long si[PRUNE_THREADS];
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    double v;
    long iv;
    prune_exact_reduce(surv, n, imu, ivar, mua, mask, par, pp, sv, si, v, iv, &bad);
    if (threadIdx.x == 0) {
        const double T = tpair[0];
        const long iT = reinterpret_cast<const long*>(tpair)[1];
        if (!better(v, iv, T, iT)) {
            v = T;
            iv = iT;
        }
        res[0] = v;
        reinterpret_cast<long*>(res)[1] = iv;
        reinterpret_cast<long*>(res)[2] = n;
        reinterpret_cast<long*>(res)[3] = bad;
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(res) + 4, res_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace boss
