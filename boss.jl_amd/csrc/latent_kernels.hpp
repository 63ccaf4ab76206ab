// latent_kernels.hpp — the latent models of a NonstationaryGP evaluated on the device (boss_nlat_*, the _lat prediction calls).
//
// In the reference λ_l(x), α(x), σ(x) are posteriors of latent ParametrizedGPs (nonstationary_gp.jl:200-214): the posterior mean
//     m(x*) = Σ_i a_i k(x_i, x*),   a = (K + σ²I)⁻¹ y,   ∇m(x*) = Σ_i a_i ∇k(x_i, x*) = Σ_i a_i α² h(r_i) (u* − u_i) ⊘ λ
// (u = x ⊘ λ, h = κ'(r)/r — kappa_r2 / kappa_prime_over_r_r2 of common.hpp, the functions kstar_rows_kernel and grad_accum_kernel
// use) pushed through Normal-cdf -> target quantile -> activation (parametrized_gp.jl:91-134), in closed form:
//     target      z = m | p0 + p1 m | exp(p0 + p1 m) | p0 + (p1 − p0) Φ(m)
//     activation  v = z | log1p(exp z) + par | exp z
// One launch covers candidate tiles × latents × members.  VALU-bound (one exp / sqrt per pair), not an MFMA job: 32 candidates
// along the lanes, the training rows of a 64-row chunk (staged through LDS with their a_i) split over 8 row subsets, 1 + d
// accumulators per lane; the subsets are summed in a fixed order (no floating-point atomics: repeated calls agree bit for bit).
// A coincident point contributes h(0) · 0 = 0 to the gradient.  The values, the chain rule and the validity check run in the same
// kernel and write λ, α, (σ), ∂λ/∂x, ∂α/∂x into the buffers the nonstationary prediction kernels read.
#pragma once
#include "common.hpp"

namespace boss {

constexpr int NLAT_MAX_D = 16;
constexpr int NLAT_CHUNK = 64;              // training rows staged through LDS at a time
constexpr int NLAT_BN = 32;                 // candidates per workgroup
constexpr int NLAT_SUBSETS = 8;             // row subsets of a chunk (256 threads)
constexpr int NLAT_T_NONE = 0, NLAT_T_NORMAL = 1, NLAT_T_LOGNORMAL = 2, NLAT_T_UNIFORM = 3;
constexpr int NLAT_A_IDENTITY = 0, NLAT_A_SOFTPLUS = 1, NLAT_A_EXP = 2;

struct NlatLatent {                         // one latent model, resident
    const double* Xsc;                      // [d][ldx] scaled training points
    const double* a;                        // [N]  (K + σ²I)⁻¹ y
    const double* invlam;                   // [d]  1 / λ
    int N, ldx, kern;                       // N = 0: the constant `cst` (no transform)
    int target, act;
    double amp2, cst, tp0, tp1, ap;
};

struct NlatJob {                            // the latents of one output and where their values at the candidates go
    const NlatLatent* lat;                  // d + 2 entries: λ_0..λ_{d-1}, α, σ
    double* clam;                           // [d][Mp]
    double* camp;                           // [Mp]
    double* cnoise;                         // [Mp] or null
    double* dlam;                           // [M][d×d], dlam[l + d (m + d j)] = ∂λ_l/∂x_m, or null
    double* damp;                           // [M][d] or null
};

// value and derivative of activation(target(m))
__device__ __forceinline__ void nlat_transform(const NlatLatent& L, double m, double& v, double& dv) {
    double z, dz;
    if (L.target == NLAT_T_NORMAL) {
        z = __builtin_fma(L.tp1, m, L.tp0);
        dz = L.tp1;
    } else if (L.target == NLAT_T_LOGNORMAL) {
        z = exp(__builtin_fma(L.tp1, m, L.tp0));
        dz = L.tp1 * z;
    } else if (L.target == NLAT_T_UNIFORM) {
        z = __builtin_fma(L.tp1 - L.tp0, normcdf_dev(m), L.tp0);
        dz = (L.tp1 - L.tp0) * normpdf_dev(m);
    } else {
        z = m;
        dz = 1.0;
    }
    if (L.act == NLAT_A_SOFTPLUS) {
        const double e = exp(-fabs(z));                      // overflow-safe: log(1 + eᶻ) = max(z, 0) + log1p(e^{−|z|})
        v = fmax(z, 0.0) + log1p(e) + L.ap;
        dv = dz * (z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e));   // sigmoid
    } else if (L.act == NLAT_A_EXP) {
        v = exp(z);
        dv = dz * v;
    } else {
        v = z;
        dv = dz;
    }
}

// grid = (Mp / 32 candidate tiles, latents, members); jobs: one per member, or null = `one` (by value: no upload for one output).
// Columns M..Mp-1 get the padding the host packing of the array calls writes (λ = 1, α = 0).  bad: smallest candidate index with an
// invalid value (integer minimum), ~0 when none.
template <bool JAC>
__global__ __launch_bounds__(256) void nlat_eval_kernel(NlatJob one, const NlatJob* __restrict__ jobs, const double* __restrict__ Craw,
                                                        int d, int Mp, int M, const unsigned char* __restrict__ discrete,
                                                        unsigned long long* __restrict__ bad) {
    __shared__ double xs[NLAT_MAX_D * NLAT_CHUNK];           // [d][chunk] scaled coordinates of the chunk's rows
    __shared__ double as[NLAT_CHUNK];
    __shared__ double red[NLAT_SUBSETS * (NLAT_MAX_D + 1) * NLAT_BN];
    const NlatJob job = jobs ? jobs[blockIdx.z] : one;
    const int q = blockIdx.y;
    const NlatLatent L = job.lat[q];
    const int tid = threadIdx.x, c = tid & 31, rs = tid >> 5;
    const int j = blockIdx.x * NLAT_BN + c;                  // < Mp
    const bool rounded = q <= d;                             // λ and α see the kernel's rounded point, σ the point as given
    double S = 0.0, G[NLAT_MAX_D];
#pragma unroll
    for (int m = 0; m < NLAT_MAX_D; ++m) G[m] = 0.0;
    if (L.N > 0 && blockIdx.x * NLAT_BN < M) {               // (uniform over the workgroup)
        double u[NLAT_MAX_D];
#pragma unroll
        for (int m = 0; m < NLAT_MAX_D; ++m) {
            u[m] = 0.0;
            if (m < d) {
                double x = Craw[(size_t)m * Mp + j];
                if (rounded && discrete && discrete[m]) x = rint(x);
                u[m] = x * L.invlam[m];
            }
        }
        for (int r0 = 0; r0 < L.N; r0 += NLAT_CHUNK) {
            __syncthreads();
            for (int idx = tid; idx < d * NLAT_CHUNK; idx += 256) {
                const int m = idx / NLAT_CHUNK, rr = idx - m * NLAT_CHUNK;
                xs[idx] = (r0 + rr < L.N) ? L.Xsc[(size_t)m * L.ldx + r0 + rr] : 0.0;
            }
            if (tid < NLAT_CHUNK) as[tid] = (r0 + tid < L.N) ? L.a[r0 + tid] : 0.0;
            __syncthreads();
#pragma unroll 2
            for (int k = 0; k < NLAT_CHUNK / NLAT_SUBSETS; ++k) {
                const int rr = rs + NLAT_SUBSETS * k;
                if (r0 + rr >= L.N) break;
                double r2 = 0.0;
#pragma unroll
                for (int m = 0; m < NLAT_MAX_D; ++m)
                    if (m < d) {
                        const double df = u[m] - xs[m * NLAT_CHUNK + rr];
                        r2 = __builtin_fma(df, df, r2);
                    }
                const double ai = as[rr];
                S = __builtin_fma(L.amp2 * kappa_r2(L.kern, r2), ai, S);
                if (JAC) {
                    const double qa = L.amp2 * kappa_prime_over_r_r2(L.kern, r2) * ai;
#pragma unroll
                    for (int m = 0; m < NLAT_MAX_D; ++m)
                        if (m < d) G[m] = __builtin_fma(qa, u[m] - xs[m * NLAT_CHUNK + rr], G[m]);
                }
            }
        }
        double* rd = red + (size_t)rs * (NLAT_MAX_D + 1) * NLAT_BN;
        rd[c] = S;
        if (JAC) {
#pragma unroll
            for (int m = 0; m < NLAT_MAX_D; ++m) rd[(1 + m) * NLAT_BN + c] = G[m];
        }
        __syncthreads();
    }
    if (rs != 0) return;
    const bool is_lam = q < d, is_amp = q == d;
    if (j >= M) {                                            // padding columns
        if (is_lam) job.clam[(size_t)q * Mp + j] = 1.0;
        else if (is_amp) job.camp[j] = 0.0;
        else if (job.cnoise) job.cnoise[j] = 0.0;
        return;
    }
    double v = L.cst, dv = 0.0;
    if (L.N > 0) {
        double m0 = 0.0;
        for (int k = 0; k < NLAT_SUBSETS; ++k) m0 += red[(size_t)k * (NLAT_MAX_D + 1) * NLAT_BN + c];   // fixed order
        nlat_transform(L, m0, v, dv);
    }
    const bool ok = is_lam ? (v > 0.0 && isfinite(v)) : (v >= 0.0 && isfinite(v));
    if (!ok) atomicMin(bad, (unsigned long long)j);
    if (is_lam) job.clam[(size_t)q * Mp + j] = v;
    else if (is_amp) job.camp[j] = v;
    else if (job.cnoise) job.cnoise[j] = v;
    if (!JAC || q > d) return;
    for (int m = 0; m < d; ++m) {
        double g = 0.0;
        if (L.N > 0 && !(discrete && discrete[m])) {
            for (int k = 0; k < NLAT_SUBSETS; ++k) g += red[((size_t)k * (NLAT_MAX_D + 1) + 1 + m) * NLAT_BN + c];
            g = dv * (g * L.invlam[m]);
        }
        if (is_lam) {
            if (job.dlam) job.dlam[q + (size_t)d * (m + (size_t)d * j)] = g;
        } else if (job.damp) {
            job.damp[m + (size_t)d * j] = g;
        }
    }
}

}  // namespace boss
