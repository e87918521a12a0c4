// grape_timegrad.hip.h -- derivative of J with respect to the time steps (ABI v7, grape_get_time_gradient).
//
// For piecewise-constant generators dU_n/d(dt_n) = -i H_n U_n, so with the states an evaluation has stored
//   dJ/d(dt_n) = -2 Re sum_k f_k <chi_k(t_{n+1})| (-i H_kn) |Psi_k(t_{n+1})>          (0-based interval n)
// where Psi_k(t_{n+1}) = U_kn Psi_k(t_n) is row n + 1 of the forward storage, chi_k(t_{n+1}) row n + 1 of the backward
// storage, and f_k the factor that turns the derivative kernels' overlaps into tau_grads: rho_k, or z_k after the
// concurrent sweeps (unit backward states).  This is _grad_J_T_via_chi! (optimize.jl:574-584) with d/d(dt_n) in place
// of d/d(eps_nl).  The built-in running cost adds the explicit derivative of its trapezoid weights,
// lambda_b / 2 sum_k (g_b,k(t_n) + g_b,k(t_{n+1})) (optimize.jl:727-750).
//
// Work as complex GEMMs over the stored state columns, per-control form: for trajectory k and a block of 16 NCT
// consecutive intervals, Y_a = O_a [Psi(t_{n0+1}) .. Psi(t_{n0+16 NCT})] for O_0 = H0_k, O_l = H_l (fp64 MFMA 16x16x4,
// four real products per complex one), contracted column by column with conj(chi) and weighted by a_ln = shape_ln eps_nl.
// The state block sits in the LDS (read once from HBM), each chi element is read once, the operators come from L2.
// The summed-operator form (one S_n per interval) would give every column an operator of its own -- a mat-vec per cell,
// not a GEMM -- so the cost here grows with (1 + L); see DESIGN.md 11.
#pragma once
#include <hip/hip_runtime.h>

struct TimeGradArgs {
    const double *H0f;    // [K][2][NP*NP] planar row-major drift
    const double *Hcf;    // [Kc][L][2][NP*NP] planar row-major control operators
    const double *eps;    // [L][N_T]
    const double *shape;  // nullptr or [L][N_T]
    const double2 *fw;    // [K][N_T+1][NP]
    const double2 *bw;    // [K][N_T+1][NP]
    const double *rho;    // [K] (z == nullptr)
    const double2 *z;     // nullptr or [K]: the backward states are the unit ones of the concurrent sweeps
    const double *gb;     // nullptr or [K][N_T+1]: g_b of the built-in running cost
    double lambda_q;      // lambda_b / 4 (the reduction multiplies by -2)
    double2 *out;         // [K][N_T]: f_k (-i q_kn) - lambda_b / 4 (g_b,k(t_n) + g_b,k(t_{n+1}))
    int K, L, N, NP, N_T, hc_per_traj;
};

// grid (ceil(N_T / (16 NCT)), K), 256 threads; dynamic LDS: 2 * NP * 16 NCT doubles (state block, planar)
template <int NCT>
__global__ void __launch_bounds__(256) time_grad_kernel(TimeGradArgs a) {
    extern __shared__ double tg_lds[];
    constexpr int CW = 16 * NCT;                    // columns (intervals) per workgroup
    const int NP = a.NP, N = a.N, N_T = a.N_T;
    const int k = blockIdx.y, n0 = blockIdx.x * CW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, lg = lane >> 4;        // MFMA: column / k-slot of A,B; D rows lg + 4 r
    double *Pr = tg_lds, *Pi = tg_lds + (size_t)NP * CW;   // [kk][CW]
    __shared__ double2 wsum[4][CW];

    // ---- the state block: Psi_k(t_{n+1}) for n = n0 .. n0 + CW - 1 (zero beyond N and beyond N_T) ----
    const double2 *fwk = a.fw + (size_t)k * (N_T + 1) * NP;
    for (int e = tid; e < NP * CW; e += 256) {
        const int c = e / NP, kk = e - c * NP;       // consecutive threads: consecutive elements of one state
        const int n = n0 + c;
        double2 v = make_double2(0., 0.);
        if (n < N_T && kk < N) v = fwk[(size_t)(n + 1) * NP + kk];
        Pr[kk * CW + c] = v.x;
        Pi[kk * CW + c] = v.y;
    }
    __syncthreads();

    const size_t pp = (size_t)NP * NP;
    const double *hck = a.Hcf + (size_t)(a.hc_per_traj ? k : 0) * a.L * 2 * pp;
    const double2 *bwk = a.bw + (size_t)k * (N_T + 1) * NP;
    double qr[NCT], qi[NCT];                          // sum over this lane's rows of conj(chi) H Psi
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) { qr[ct] = 0.; qi[ct] = 0.; }

    const int RT = NP / 16, KS = NP / 4;
    for (int rt = wave; rt < RT; rt += 4) {
        // chi of this lane's four rows and its columns: read once
        double cr[NCT][4], ci[NCT][4];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int n = n0 + 16 * ct + lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * rt + lg + 4 * r;
                double2 v = make_double2(0., 0.);
                if (n < N_T && row < N) v = bwk[(size_t)(n + 1) * NP + row];
                cr[ct][r] = v.x; ci[ct][r] = v.y;
            }
        }
        for (int op = 0; op <= a.L; ++op) {
            const double *O = op == 0 ? a.H0f + (size_t)k * 2 * pp : hck + (size_t)(op - 1) * 2 * pp;
            double coef[NCT];                         // a_ln of this lane's columns (the drift: 1)
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int n = min(n0 + 16 * ct + lc, N_T - 1);
                const size_t ln = (size_t)max(op - 1, 0) * N_T + n;   // (op 0: not read)
                coef[ct] = op == 0 ? 1.0 : a.eps[ln] * (a.shape ? a.shape[ln] : 1.0);
            }
            const double *Ore = O + (size_t)(16 * rt + lc) * NP + lg, *Oim = Ore + pp;
            d4 yr[NCT], yi[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) { yr[ct] = d4{0., 0., 0., 0.}; yi[ct] = d4{0., 0., 0., 0.}; }
            for (int ks = 0; ks < KS; ++ks) {
                const double ar = Ore[4 * ks], ai = Oim[4 * ks];   // A[row 16 rt + lc][kk = 4 ks + lg]
                const int kk = 4 * ks + lg;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const double br = Pr[kk * CW + 16 * ct + lc], bi = Pi[kk * CW + 16 * ct + lc];   // B[kk][column]
                    yr[ct] = MFMA64(ar, br, yr[ct]);
                    yr[ct] = MFMA64(-ai, bi, yr[ct]);
                    yi[ct] = MFMA64(ar, bi, yi[ct]);
                    yi[ct] = MFMA64(ai, br, yi[ct]);
                }
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                double sr = 0., si = 0.;
#pragma unroll
                for (int r = 0; r < 4; ++r) {   // D[row lg + 4 r][column lc]
                    sr += cr[ct][r] * yr[ct][r] + ci[ct][r] * yi[ct][r];
                    si += cr[ct][r] * yi[ct][r] - ci[ct][r] * yr[ct][r];
                }
                qr[ct] = fma(coef[ct], sr, qr[ct]);
                qi[ct] = fma(coef[ct], si, qi[ct]);
            }
        }
    }
    // ---- rows of the four lane groups, then of the four waves, in a fixed order ----
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        qr[ct] += __shfl_xor(qr[ct], 16, 64);
        qi[ct] += __shfl_xor(qi[ct], 16, 64);
        qr[ct] += __shfl_xor(qr[ct], 32, 64);
        qi[ct] += __shfl_xor(qi[ct], 32, 64);
        if (lg == 0) wsum[wave][16 * ct + lc] = make_double2(qr[ct], qi[ct]);
    }
    __syncthreads();
    if (tid < CW) {
        const int n = n0 + tid;
        if (n < N_T) {
            double q_r = 0., q_i = 0.;
#pragma unroll
            for (int w = 0; w < 4; ++w) { q_r += wsum[w][tid].x; q_i += wsum[w][tid].y; }
            const double wr = q_i, wi = -q_r;            // -i q
            double2 v;
            if (a.z) {
                const double2 zk = a.z[k];
                v = make_double2(zk.x * wr - zk.y * wi, zk.x * wi + zk.y * wr);
            } else {
                const double rk = a.rho[k];
                v = make_double2(rk * wr, rk * wi);
            }
            if (a.gb) v.x -= a.lambda_q * (a.gb[(size_t)k * (N_T + 1) + n] + a.gb[(size_t)k * (N_T + 1) + n + 1]);
            a.out[(size_t)k * N_T + n] = v;
        }
    }
}
