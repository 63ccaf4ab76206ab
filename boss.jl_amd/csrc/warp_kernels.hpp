// warp_kernels.hpp — warps (boss_warp_t): the input warp x -> x_ and the output transform (y_, std_) -> (y, std) of a TransformedModel
// (src/models/transformed.jl:222-257,330-378), both traced into mean programs with T = 0 and interpreted by fit_eval / fit_grad of
// fitness.hpp.  Two stages: the candidates are warped on the device (with ∂x_/∂x from the reverse sweeps), and the model-space
// moments (μ_, σ²_, ∇μ_, ∇σ²_) of every posterior sample are pushed through the output programs and both Jacobians back to user
// space.  The arithmetic around the interpreter is written once, as the __host__ __device__ functions below, for the kernels and
// their host twins (host_warp.inc).
#pragma once
#include "mean_program.hpp"

namespace boss {

constexpr int WARP_MAXD = 16;                                // d_user, d_model
constexpr int WARP_MAXP = 8;                                 // outputs under an output program: 2P <= 16 program outputs
constexpr int WARP_MAX_WAVES = 4;

// LDS doubles per thread.  Input warp: a mean program's column over d_user inputs, y[d] | v[nI] (| ay[d] | av[nI]), shared by the
// d_model programs of a point, which run one after the other in its thread.  Moments: y[2P] = (μ_, σ_) | v[nI] (| ay[2P] | av[nI] |
// g[d_model], the model-space gradient of the thread's output row before Jᵀ is applied).
__host__ __device__ constexpr int warp_x_slots(int d_user, int nI, bool grad) { return mean_slots(d_user, nI, grad); }
__host__ __device__ constexpr int warp_m_slots(int P, int nI, int d_model, bool grad) {
    return mean_slots(2 * P, nI, grad) + (grad ? d_model : 0);
}
// The longest cases, one wave each: 16 inputs and 64 instructions with the sweep are 160 slots = 80 KiB; 2P = 16 moments, 64
// instructions, the sweep and 16 gradient slots are 176 slots = 88 KiB.
constexpr int WARP_X_MAX_LDS = 64 * (int)sizeof(double) * warp_x_slots(WARP_MAXD, FIT_MAXI, true);
constexpr int WARP_M_MAX_LDS = 64 * (int)sizeof(double) * warp_m_slots(WARP_MAXP, FIT_MAXI, WARP_MAXD, true);

// One point of the input warp: x (d_user values, contiguous) -> xo (d_model values, xs apart) and, with GRAD, Jj = ∂x_/∂x,
// d_model×d_user column-major (Jj[r + d_model*k] = ∂x_r/∂x_k).  col: the point's column of warp_x_slots doubles, stride st.
template <bool GRAD>
__host__ __device__ inline void warp_x_point(const FitProg* __restrict__ gin, int d_user, int d_model, int nI_max,
                                             const double* __restrict__ x, double* __restrict__ col, int st, double* __restrict__ xo,
                                             size_t xs, double* __restrict__ Jj) {
    double* cy = col;
    double* cv = cy + (size_t)d_user * st;
    double* cay = cv + (size_t)nI_max * st;
    double* cav = cay + (size_t)d_user * st;
    for (int k = 0; k < d_user; ++k) cy[(size_t)k * st] = x[k];
    for (int r = 0; r < d_model; ++r) {
        double val;
        [[clang::always_inline]] val = fit_eval(gin[r], cy, cv, st);   // (a call would bring a stack frame: scratch memory)
        xo[(size_t)r * xs] = val;
        if (GRAD) {
            [[clang::always_inline]] fit_grad(gin[r], cy, cv, cay, cav, st);
            for (int k = 0; k < d_user; ++k) Jj[r + (size_t)d_model * k] = cay[(size_t)k * st];
        }
    }
}

// One (candidate j, output row r) of one posterior sample.  Rows 0..P-1 are the means, rows P..2P-1 the standard deviations: row r
// writes mu[p] (and dmu[p]) or var[p] (and dvar[p]) of output p = r mod P and nothing else.
//   mu_s, var_s [p][M] model-space moments; dmu_s, dvar_s [p][d_model×M] (k' + d_model*j) their gradients w.r.t. x_ (GRAD);
//   Jj          ∂x_/∂x at candidate j (d_model×d_user column-major) or NULL = the identity (then d_model == d_user);
//   gout        the 2P output programs over (μ_0.., σ_0..), or NULL = the identity: moments pass through bit for bit, only Jᵀ is applied;
//   mu_o, var_o [p][M]; dmu_o, dvar_o [p][d_user×M] (k + d_user*j).
// σ_ = sqrt(σ²_) with a variance in [-1e-8, 0) clipped to 0; ∇σ_ = ∇σ²_/(2σ_), and 0 where the variance was clipped or is 0.
// (μ, σ) = out(μ_, σ_), σ² = σ·σ whatever the sign of σ (transformed.jl:343,350), ∇_{x_} out_r = Σ_q ∂out_r/∂μ_q ∇μ_q + ∂out_r/∂σ_q ∇σ_q
// in ascending q, ∇_x = Jᵀ ∇_{x_} in ascending k', ∇σ² = 2σ∇σ.  A variance below -1e-8 anywhere in the sample's column poisons the
// candidate: its moments pass through untouched (the caller's test for that variance still fires) with zero gradients.
template <bool GRAD>
__host__ __device__ inline void warp_moments_point(const FitProg* __restrict__ gout, int P, int r, int nI_max, int M, int d_model,
                                                   int d_user, const double* __restrict__ mu_s, const double* __restrict__ var_s,
                                                   const double* __restrict__ dmu_s, const double* __restrict__ dvar_s,
                                                   const double* __restrict__ Jj, int j, double* __restrict__ col, int st,
                                                   double* __restrict__ mu_o, double* __restrict__ var_o, double* __restrict__ dmu_o,
                                                   double* __restrict__ dvar_o) {
    const bool is_sd = r >= P;
    const int p = is_sd ? r - P : r;
    const size_t dmM = (size_t)d_model * M, duM = (size_t)d_user * M;
    double* cy = col;
    double* cv = cy + (size_t)2 * P * st;
    double* cay = cv + (size_t)nI_max * st;
    double* cav = cay + (size_t)2 * P * st;
    double* cg = cav + (size_t)nI_max * st;
    double* go = GRAD ? (is_sd ? dvar_o : dmu_o) + (size_t)p * duM + (size_t)j * d_user : nullptr;
    bool poison = false;
    for (int q = 0; q < P; ++q) {
        double v = var_s[(size_t)q * M + j];
        if (v < 0.0) {
            if (v < -MAX_NEG_VAR) poison = true;
            v = 0.0;
        }
        if (gout) {                                          // (the identity reads neither)
            cy[(size_t)q * st] = mu_s[(size_t)q * M + j];
            cy[(size_t)(P + q) * st] = sqrt(v);
        }
    }
    if (poison || !gout) {
        if (is_sd) var_o[(size_t)p * M + j] = var_s[(size_t)p * M + j];
        else mu_o[(size_t)p * M + j] = mu_s[(size_t)p * M + j];
        if (!GRAD) return;
        if (poison) {
            for (int k = 0; k < d_user; ++k) go[k] = 0.0;
            return;
        }
        const double* gi = (is_sd ? dvar_s : dmu_s) + (size_t)p * dmM + (size_t)j * d_model;
        for (int k = 0; k < d_user; ++k) {
            if (!Jj) {
                go[k] = gi[k];
                continue;
            }
            double acc = 0.0;
            for (int kk = 0; kk < d_model; ++kk) acc += Jj[kk + (size_t)d_model * k] * gi[kk];
            go[k] = acc;
        }
        return;
    }
    double val;
    [[clang::always_inline]] val = fit_eval(gout[r], cy, cv, st);
    if (is_sd) var_o[(size_t)p * M + j] = val * val;
    else mu_o[(size_t)p * M + j] = val;
    if (!GRAD) return;
    [[clang::always_inline]] fit_grad(gout[r], cy, cv, cay, cav, st);
    for (int kk = 0; kk < d_model; ++kk) {
        double acc = 0.0;
        for (int q = 0; q < P; ++q) {
            const double sd = cy[(size_t)(P + q) * st];
            const double gm = dmu_s[(size_t)q * dmM + (size_t)j * d_model + kk];
            const double gs = sd > 0.0 ? dvar_s[(size_t)q * dmM + (size_t)j * d_model + kk] / (2.0 * sd) : 0.0;
            acc += cay[(size_t)q * st] * gm;
            acc += cay[(size_t)(P + q) * st] * gs;
        }
        cg[(size_t)kk * st] = acc;
    }
    const double scale = is_sd ? 2.0 * val : 1.0;
    for (int k = 0; k < d_user; ++k) {
        double acc;
        if (Jj) {
            acc = 0.0;
            for (int kk = 0; kk < d_model; ++kk) acc += Jj[kk + (size_t)d_model * k] * cg[(size_t)kk * st];
        } else
            acc = cg[(size_t)k * st];
        go[k] = is_sd ? scale * acc : acc;
    }
}

#ifdef __HIPCC__
// One thread per candidate; its d_model programs (a device buffer, uniform loads) run one after the other on one LDS column sized
// at launch from the actual programs (warp_x_slots).  Coordinate r of candidate j goes to X_[r*xs_r + j*xs_j]: (1, d_model) is d_model×M
// column-major, (Mp, 1) the dimension-major rows of a candidate buffer (boss_cand), written straight into it.  J candidate after
// candidate.  No atomics, no barrier: threads behind the last candidate leave.
template <bool GRAD>
__global__ __launch_bounds__(64 * WARP_MAX_WAVES) void warp_x_kernel(const FitProg* __restrict__ gin, const double* __restrict__ Xs, int M,
                                                                      int d_user, int d_model, int nI_max, double* __restrict__ X_,
                                                                      size_t xs_r, size_t xs_j, double* __restrict__ J) {
    extern __shared__ __attribute__((aligned(16))) char warp_lds_raw[];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    double* col = reinterpret_cast<double*>(warp_lds_raw) + threadIdx.x;
    warp_x_point<GRAD>(gin, d_user, d_model, nI_max, Xs + (size_t)j * d_user, col, (int)blockDim.x, X_ + (size_t)j * xs_j, xs_r,
                       GRAD ? J + (size_t)j * d_model * d_user : nullptr);
}

// One thread per (candidate j, output row blockIdx.y, sample s): grid = candidate tiles × rows × min(S, 65535), samples beyond the
// grid's z extent in a stride loop.  rows = 2P (P with only the means asked for is not offered: both moments always travel).
// Sample s sits s·P·M behind mu_ / var_ / mu / var, s·P·d_model·M behind dmu_ / dvar_, s·P·d_user·M behind dmu / dvar.
template <bool GRAD>
__global__ __launch_bounds__(64 * WARP_MAX_WAVES) void warp_moments_kernel(const FitProg* __restrict__ gout, int P, int nI_max, int S, int M,
                                                                            int d_model, int d_user, const double* __restrict__ mu_,
                                                                            const double* __restrict__ var_, const double* __restrict__ dmu_,
                                                                            const double* __restrict__ dvar_, const double* __restrict__ J,
                                                                            double* __restrict__ mu, double* __restrict__ var,
                                                                            double* __restrict__ dmu, double* __restrict__ dvar) {
    extern __shared__ __attribute__((aligned(16))) char warp_lds_raw[];
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    double* col = reinterpret_cast<double*>(warp_lds_raw) + threadIdx.x;
    const int r = blockIdx.y;
    const size_t pm = (size_t)P * M, pdm = pm * d_model, pdu = pm * d_user;
    const double* Jj = J ? J + (size_t)j * d_model * d_user : nullptr;
    for (int s = blockIdx.z; s < S; s += gridDim.z)
        warp_moments_point<GRAD>(gout, P, r, nI_max, M, d_model, d_user, mu_ + s * pm, var_ + s * pm, GRAD ? dmu_ + s * pdm : nullptr,
                                 GRAD ? dvar_ + s * pdm : nullptr, Jj, j, col, (int)blockDim.x, mu + s * pm, var + s * pm,
                                 GRAD ? dmu + s * pdu : nullptr, GRAD ? dvar + s * pdu : nullptr);
}
#endif  // __HIPCC__

}  // namespace boss
