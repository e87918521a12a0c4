// grape_hvp_split.hip.h -- the Hessian-vector product of grape_hvp.hip.h cut at its one cross-trajectory dependency
// (grape_hvp_forward / grape_hvp_backward / grape_hvp_backward_chi).
//
// grape_hvp runs tangent forward sweep, boundary, backward sweep in one call.  Between the sweeps sits the only quantity
// that couples the trajectories, f' = sum_k w_k tau'_k, and the only place where the functional enters, the boundary
// chi_k(T) = c_k tgt_k, chi'_k(T) = c'_k tgt_k.  A trajectory shard (K < K_total) has to all-reduce f' on the host, a caller's
// functional has to supply chi and chi' itself.  So:
//   forward half : hvp_forward_kernel as it is, then hvp_partial_sum_kernel: sum_k w_k tau'_k of THIS handle's trajectories
//   built-in     : hvp_coef_total_kernel fills c'_k from the all-reduced f', then hvp_backward_kernel as it is (its f is a
//                  pointer: it reads the all-reduced f the caller passed)
//   caller's chi : hvp_backward_chi_kernel -- hvp_backward_kernel restated with columns 0 and 1 of the block loaded from
//                  chi~ [K][NP] and chi~' [nd][K][NP] (balanced frame, padded rows zero) instead of formed as c tgt.
// The two small kernels repeat the loops and expressions of hvp_boundary_kernel, so that on an unsharded handle the two
// halves give the bits of grape_hvp.  The restated sweep shares hvp_build_step, hvp_series_step and hvp_column with the
// original (same LDS, two barriers per term, fixed-order reductions, no atomics on floating point, no scratch); the
// original is not routed through a shared body.
#pragma once
#include "grape_hvp.hip.h"

// ---------------------------------------------------------------------------------------
// sum_k w_k tau'_k over the trajectories of this handle: grid (directions), one wave; psums [nd][2]
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) hvp_partial_sum_kernel(HvpArgs a, double *psums) {
    const int j = blockIdx.x, lane = threadIdx.x, K = a.K;
    const double2 *dt = a.dtau + (size_t)j * K;
    double fr = 0., fi = 0.;
    for (int k = lane; k < K; k += 64) {
        const double w = a.weights ? a.weights[k] : 1.0;
        fr += w * dt[k].x; fi += w * dt[k].y;
    }
    fr = wave_sum(fr); fi = wave_sum(fi);
    if (lane == 0) { psums[2 * j] = fr; psums[2 * j + 1] = fi; }
}

// ---------------------------------------------------------------------------------------
// Psi~'_k(T) of every (direction, trajectory), packed for ONE copy to the host on the handle's stream: out [nd K][N].
// Grid (nd K), one wave.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) hvp_final_tangent_kernel(HvpArgs a, int NP, double2 *out) {
    const size_t wg = blockIdx.x;
    const double2 *src = a.dpsi + (wg * (size_t)(a.N_T + 1) + (size_t)a.N_T) * NP;
    for (int i = threadIdx.x; i < a.N; i += 64) out[wg * a.N + i] = src[i];
}

// ---------------------------------------------------------------------------------------
// c'_k of chi'_k(T) = c'_k tgt_k from the all-reduced f' (df_total [nd][2]): grid (directions), one wave
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) hvp_coef_total_kernel(HvpArgs a, const double *df_total) {
    const int j = blockIdx.x, lane = threadIdx.x, K = a.K;
    const double2 *dt = a.dtau + (size_t)j * K;
    const double fr = df_total[2 * j], fi = df_total[2 * j + 1];
    const double Kt = (double)a.K_total;
    for (int k = lane; k < K; k += 64) {
        const double w = a.weights ? a.weights[k] : 1.0;
        double2 c = make_double2(0., 0.);
        if (a.functional == 0) c = make_double2(w * fr / (Kt * Kt), w * fi / (Kt * Kt));
        else if (a.functional == 1) c = make_double2(w * dt[k].x / Kt, w * dt[k].y / Kt);
        a.dcoef[(size_t)j * K + k] = c;
    }
}

// ---------------------------------------------------------------------------------------
// Backward sweep from the caller's boundary: grid (K, directions), NP / 16 waves, NCT column tiles (2 + 2L columns).
// chi [K][NP], dchi [nd][K][NP]: balanced frame, rows N..NP-1 zero.  Reads neither targets, weights, tau, f nor the functional.
// ---------------------------------------------------------------------------------------
template <int NP, int NCT>
__global__ void __launch_bounds__(4 * NP) hvp_backward_chi_kernel(HvpArgs a, const double2 *chi, const double2 *dchi) {
    constexpr int NW = NP / 16, NTH = 64 * NW, NP2 = NP * NP, CW = 16 * NCT;
    __shared__ double Xr[NP * CW], Xi[NP * CW];
    __shared__ double red[NW][2][CW];
    __shared__ double dscale[8];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, j = blockIdx.y, N = a.N, N_T = a.N_T, L = a.L;
    const size_t wg = (size_t)j * a.K + k;
    double *Am = a.ws + wg * 4 * NP2, *Bm = Am + 2 * NP2;
    const double *Hc = a.Hcf + (size_t)(a.hc_per_traj ? k : 0) * L * 2 * NP2;
    const double *v = a.V + (size_t)j * L * N_T;
    const double2 *fwk = a.fw + (size_t)k * (N_T + 1) * NP;
    const double2 *dps = a.dpsi + wg * (size_t)(N_T + 1) * NP;
    double2 *tg = a.tg + wg * (size_t)L * N_T;
    HvpCol col[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) col[ct] = hvp_column<true>(16 * ct + lc, L);

    // c = chi~_k(T), c' = chi~'_k(T) as the caller gave them; p = p' = 0
    d4 sr[NCT], si[NCT];
    {
        const double2 *c0 = chi + (size_t)k * NP, *c1 = dchi + wg * (size_t)NP;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg, q = 16 * ct + lc;
                double2 x = make_double2(0., 0.);
                if (q == 0) x = c0[row];
                else if (q == 1) x = c1[row];
                sr[ct][r] = x.x; si[ct][r] = x.y;
                Xr[row * CW + q] = x.x; Xi[row * CW + q] = x.y;
            }
    }
    int maxo = HVP_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    for (int n = N_T - 1; n >= 0; --n) {
        double dt;
        const int msub = hvp_build_step<NP, NTH, true>(a, k, n, v, Am, Bm, dt);
        if (tid < L) dscale[tid] = (a.shape ? a.shape[(size_t)tid * N_T + n] : 1.0) * dt;
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            const int na = hvp_series_step<NP, NCT, true>(a, Am, Bm, Hc, dscale, Xr, Xi, red, sr, si, col, wave, lane, maxo);
            if (na < 0) { failed = true; maxo = 1; } else terms += (unsigned long long)na;
            ++substeps;
        }
        // <P_l | Psi'(t_n)> + <P'_l | Psi(t_n)>: rows of a lane, lane groups, then waves in index order
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int q = 16 * ct + lc;
            const bool isp = q >= 2 && q < 2 + L, ispp = q >= 2 + L && q < 2 + 2 * L;
            double dr = 0., di = 0.;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg;
                double2 x = make_double2(0., 0.);
                if (row < N) {
                    if (isp) x = dps[(size_t)n * NP + row];
                    else if (ispp) x = fwk[(size_t)n * NP + row];
                }
                dr += sr[ct][r] * x.x + si[ct][r] * x.y;
                di += sr[ct][r] * x.y - si[ct][r] * x.x;
            }
            dr += __shfl_xor(dr, 16, 64); di += __shfl_xor(di, 16, 64);
            dr += __shfl_xor(dr, 32, 64); di += __shfl_xor(di, 32, 64);
            if (lg == 0) { red[wave][0][q] = dr; red[wave][1][q] = di; }
        }
        __syncthreads();
        if (tid < L) {
            double dr = 0., di = 0.;
            for (int w = 0; w < NW; ++w) {
                dr += red[w][0][2 + tid] + red[w][0][2 + L + tid];
                di += red[w][1][2 + tid] + red[w][1][2 + L + tid];
            }
            tg[(size_t)tid * N_T + n] = make_double2(dr, di);
        }
        // p = p' = 0 for the next interval; c, c' carry on
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int q = 16 * ct + lc;
            if (q >= 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * wave + 4 * r + lg;
                    sr[ct][r] = 0.; si[ct][r] = 0.;
                    Xr[row * CW + q] = 0.; Xi[row * CW + q] = 0.;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        const size_t s = (size_t)gridDim.x * gridDim.y + wg;
        a.stats[2 * s] = terms;
        a.stats[2 * s + 1] = substeps;
    }
}
