// grape_hessian.hip.h -- the exact Hessian of J as a matrix on the stored forward states (grape_hessian, N <= 64, L <= 4).
//
// grape_hvp gives H v; nv = L N_T unit directions give H, but a unit direction e_(m,l') spends a whole 16-column tile and two
// full sweeps on a tangent that is zero before t_m and merely propagated after t_{m+1}.  Written out per trajectory, with
// 0-based intervals and U_n: t_n -> t_{n+1},
//     A_n = -i dt_n H_kn,   D_nl = -i dt_n s_ln H_l                            (as grape_hvp.hip.h)
//     theta_k(T) = tgt_k,   theta_k(t_n) = U_n^dagger theta_k(t_{n+1})         the BARE target chain (defined when c_k = 0)
//     a_(n,l)    = DU_n[D_nl] Psi_k(t_n)                                       lives at t_{n+1}
//     beta_(n,l) = DU_n[D_nl]^dagger theta_k(t_{n+1})                          lives at t_n
//     T_k,p      = d tau_k / d eps_p = <beta_p | Psi_k(t_n)>                   p = (n, l)
//     S_k,pq     = <beta_(n,l) | U_{n-1} ... U_{m+1} a_(m,l')>                 m < n  (empty product for n = m + 1)
//                = <theta_k(t_{n+1}) | D^2U_n[D_nl, D_nl'] Psi_k(t_n)>         m = n;   symmetric in p <-> q
//     H_pq = -2 Re sum_k [ conj(c_k) S_k,pq + conj(d_q c_k) T_k,p ]            chi_k(T) = c_k tgt_k (include/grape_hip.h)
//            sm: d_q c_k = w_k F_q / K_total^2, F_q = sum_j w_j T_j,q;   ss: d_q c_k = w_k T_k,q / K_total;   re: 0
// the part off the diagonal blocks is a FAN: the L N_T columns a_(m,l') are carried forwards as 16-column blocks, each block
// from the interval where its first column is born, and overlapped with the L vectors beta_(n,.) at every grid point.
//
//   hess_forward_seeds_kernel   grid (K, G): block (k, g) takes the intervals n = g, g + G, ... (independent: Psi_k(t_n) is
//                               stored).  Columns [u a_1..a_L]:  u_{j+1} = A u_j / (j+1),  a_{j+1} = (A a_j + D_l u_j) / (j+1).
//   hess_backward_seeds_kernel  grid (K), sequential in n from the bare target.  Columns [theta beta_1..beta_L beta2_(l'<=l)],
//                               1 + L + L (L + 1) / 2 <= 15 columns for L <= 4 (one tile: the limit on L):
//                               beta_{j+1} = (A^+ beta_j + D_l^+ theta_j) / (j+1),
//                               beta2_{j+1} = (A^+ beta2_j + D_l^+ beta_l',j + D_l'^+ beta_l,j) / (j+1).
//                               Stores beta, T = <beta | Psi(t_n)>, S_diag = <beta2 | Psi(t_n)>; clears beta, beta2; theta carries on.
//   hess_fan_kernel             grid (ceil(L N_T / 16), trajectories of the pass).  Columns interval-major, q = m L + l'.  At
//                               every n from the birth of the first column: load the columns born at t_n, write
//                               Re(conj(c_k) <beta_(n,l) | x_q>) for every live column and every l into the strip of the
//                               trajectory, propagate through interval n (not the last one).
//   hess_accumulate_kernel      adds the strips of a pass into the accumulator in ascending k, one after the other: the bits
//                               do not depend on how the trajectories are cut into passes.
//   hess_finish_kernel          diagonal blocks and boundary term in a fixed order over k, times -2, the lower triangle
//                               mirrored, (n, l) -> p = l N_T + n.
// Series as in grape_hvp.hip.h: m = ceil(beta_n dt_n / theta) sub-steps with all chains carried over, a series stops when
// EVERY column has ||term|| <= tol ||sum|| (an identically zero column counts as converged), after at most HVP_MAX_ORDER
// terms (flag 16 otherwise).  Layout as there: NP / 16 waves, wave w owns the rows [16 w, 16 w + 16) of every column, the
// term block planar in the LDS, the sums in the registers of the owning lane, two barriers per term, norms reduced lane
// groups first, then waves in index order.  No atomics except the flag word.  No scratch memory.
#pragma once
#include "grape_hvp.hip.h"

#define HESS_MAX_L 4
#define HESS_PAIRS 10   // L (L + 1) / 2 at L = 4: the stride of the diagonal-block overlaps

struct HessArgs {
    HvpArgs s;              // static data, stored states, tau, f, flags, tol, theta and sizes as grape_hvp reads them
    double2 *av;            // [K][N_T][L][NP] a_(n,l)
    double2 *bv;            // [K][N_T][L][NP] beta_(n,l)
    double2 *T;             // [K][N_T*L] T_k,(n,l)
    double2 *Sd;            // [K][N_T][HESS_PAIRS] S_k,(n,l)(n,l'), pair l (l + 1) / 2 + l', l' <= l
    double *strip;          // [trajectories of the pass][P][P] rows (n, l), columns (m, l'); written for m < n only
    double *acc;            // [P][P] sum over the trajectories so far (m < n only)
    double *H;              // [P][P] the result, p = l N_T + n
    double *ws;             // [workgroups][2][2][NP*NP] step matrices
    unsigned long long *stats;   // [workgroups][2] series terms, (sub-)steps of the launch
    int k0;                 // first trajectory of the pass
};

// What D_l of the step does for the lane's column q: it multiplies column src[l] of the term block into q, fac[l] times.
struct HessCol {
    int src[HESS_MAX_L];
    double fac[HESS_MAX_L];
    double self;
};
// MODE 0: [u a_1..a_L];  MODE 1: [theta beta_1..beta_L beta2_(l'<=l)];  MODE 2: sixteen independent columns
template <int MODE>
__device__ __forceinline__ HessCol hess_column(const int q, const int L) {
    HessCol c;
#pragma unroll
    for (int l = 0; l < HESS_MAX_L; ++l) { c.src[l] = 0; c.fac[l] = 0.; }
    c.self = 1.;
    if (MODE == 0) {
        c.self = q <= L ? 1. : 0.;
#pragma unroll
        for (int l = 0; l < HESS_MAX_L; ++l)
            if (q == 1 + l && l < L) c.fac[l] = 1.;
    } else if (MODE == 1) {
        c.self = q < 1 + L + L * (L + 1) / 2 ? 1. : 0.;
#pragma unroll
        for (int l = 0; l < HESS_MAX_L; ++l) {
            if (l >= L) continue;
            if (q == 1 + l) c.fac[l] = 1.;
#pragma unroll
            for (int l2 = 0; l2 <= l; ++l2) {
                if (q != 1 + L + l * (l + 1) / 2 + l2) continue;
                if (l2 == l) { c.src[l] = 1 + l; c.fac[l] = 2.; }
                else { c.src[l] = 1 + l2; c.fac[l] = 1.; c.src[l2] = 1 + l; c.fac[l2] = 1.; }
            }
        }
    }
    return c;
}

// One (sub-)step of the block series on one column tile (the pattern of hvp_series_step).  On entry X holds the start
// vectors and (sr, si) the same values; on exit both hold the sums.  Returns the number of terms, or -1.
template <int NP, int MODE>
__device__ __forceinline__ int hess_series_step(const HessArgs &a, const double *Am, const double *Hc, const double *dscale, double *Xr,
                                                double *Xi, double (*red)[2][16], d4 &sr, d4 &si, const HessCol &col, const int wave,
                                                const int lane, const int maxo) {
    constexpr int CW = 16, NW = NP / 16, NP2 = NP * NP;
    const int lc = lane & 15, lg = lane >> 4;
    const double tol2 = a.s.tol * a.s.tol;
    bool conv = false;
    int aord = 0;
    for (; aord < maxo && !conv; ++aord) {
        const double fac = c_series_inv[aord & 255];
        d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
        hvp_mac<NP, CW, false>(cr, ci, Am, wave, lane, Xr, Xi, lc, col.self, 0.);
        if (MODE != 2) {
#pragma unroll
            for (int l = 0; l < HESS_MAX_L; ++l) {
                if (l >= a.s.L) continue;
                // D_l = (-i s dt) H_l;  D_l^dagger = (i s dt) H_l^dagger
                if (MODE == 0) hvp_mac<NP, CW, false>(cr, ci, Hc + (size_t)l * 2 * NP2, wave, lane, Xr, Xi, col.src[l], 0., -col.fac[l] * dscale[l]);
                else hvp_mac<NP, CW, true>(cr, ci, Hc + (size_t)l * 2 * NP2, wave, lane, Xr, Xi, col.src[l], 0., col.fac[l] * dscale[l]);
            }
        }
        d4 tr, tim;
        double t2 = 0., s2 = 0.;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double ur = fac * cr[r], ui = fac * ci[r];
            tr[r] = ur; tim[r] = ui;
            sr[r] += ur; si[r] += ui;
            t2 += ur * ur + ui * ui;
            s2 += sr[r] * sr[r] + si[r] * si[r];
        }
        t2 += __shfl_xor(t2, 16, 64); s2 += __shfl_xor(s2, 16, 64);
        t2 += __shfl_xor(t2, 32, 64); s2 += __shfl_xor(s2, 32, 64);
        if (lg == 0) { red[wave][0][lc] = t2; red[wave][1][lc] = s2; }
        __syncthreads();   // every wave has read the old terms; the norms are visible
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (16 * wave + 4 * r + lg) * CW + lc;
            Xr[o] = tr[r]; Xi[o] = tim[r];
        }
        bool ok = true;
        if (lane < CW) {
            double u2 = 0., v2 = 0.;
#pragma unroll
            for (int w = 0; w < NW; ++w) { u2 += red[w][0][lane]; v2 += red[w][1][lane]; }
            ok = u2 <= tol2 * v2;   // (0 <= 0: an identically zero column has converged)
        }
        conv = __ballot(!ok) == 0ull;
        __syncthreads();   // the new terms are visible; the norms have been read
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = (16 * wave + 4 * r + lg) * CW + lc;
        Xr[o] = sr[r]; Xi[o] = si[r];
    }
    __syncthreads();
    return conv ? aord : -1;
}

// c_k of chi_k(T) = c_k tgt_k at the last evaluation (include/grape_hip.h)
__device__ __forceinline__ double2 hess_coef(const HvpArgs &s, const int k) {
    const double w = s.weights ? s.weights[k] : 1.0, Kt = (double)s.K_total;
    if (s.functional == 0) return make_double2(w * s.f[0] / (Kt * Kt), w * s.f[1] / (Kt * Kt));
    if (s.functional == 1) { const double2 t = s.tau[k]; return make_double2(w * t.x / Kt, w * t.y / Kt); }
    return make_double2(w / (2.0 * Kt), 0.);
}

// ---------------------------------------------------------------------------------------
// Forward seeds a_(n,l) = DU_n[D_nl] Psi_k(t_n): grid (K, G), NP / 16 waves; block (k, g) takes n = g, g + G, ...
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(4 * NP) hess_forward_seeds_kernel(HessArgs a) {
    constexpr int NW = NP / 16, NTH = 64 * NW, NP2 = NP * NP, CW = 16;
    __shared__ double Xr[NP * CW], Xi[NP * CW];
    __shared__ double red[NW][2][CW];
    __shared__ double dscale[HESS_MAX_L];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, N = a.s.N, N_T = a.s.N_T, L = a.s.L;
    const size_t wg = (size_t)blockIdx.y * gridDim.x + k;
    double *Am = a.ws + wg * 4 * NP2, *Bm = Am + 2 * NP2;
    const double *Hc = a.s.Hcf + (size_t)(a.s.hc_per_traj ? k : 0) * L * 2 * NP2;
    const double2 *fwk = a.s.fw + (size_t)k * (N_T + 1) * NP;
    const HessCol col = hess_column<0>(lc, L);
    int maxo = HVP_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    for (int n = blockIdx.y; n < N_T; n += gridDim.y) {
        d4 sr, si;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * wave + 4 * r + lg;
            double2 x = make_double2(0., 0.);
            if (lc == 0 && row < N) x = fwk[(size_t)n * NP + row];
            sr[r] = x.x; si[r] = x.y;
            Xr[row * CW + lc] = x.x; Xi[row * CW + lc] = x.y;
        }
        double dt;
        // (the direction operand of hvp_build_step is not used here: the pulses stand in for it, Bm is never read)
        const int msub = hvp_build_step<NP, NTH, false>(a.s, k, n, a.s.eps, Am, Bm, dt);
        if (tid < L) dscale[tid] = (a.s.shape ? a.s.shape[(size_t)tid * N_T + n] : 1.0) * dt;
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            const int na = hess_series_step<NP, 0>(a, Am, Hc, dscale, Xr, Xi, red, sr, si, col, wave, lane, maxo);
            if (na < 0) { failed = true; maxo = 1; } else terms += (unsigned long long)na;
            ++substeps;
        }
        if (lc >= 1 && lc <= L) {
            double2 *out = a.av + (((size_t)k * N_T + n) * L + (lc - 1)) * NP;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[16 * wave + 4 * r + lg] = make_double2(sr[r], si[r]);
        }
        __syncthreads();   // (dscale and the term block are rewritten for the next interval)
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.s.flags[0], 16);
        a.stats[2 * wg] = terms;
        a.stats[2 * wg + 1] = substeps;
    }
}

// ---------------------------------------------------------------------------------------
// Backward seeds: grid (K), NP / 16 waves, sequential in n from the bare target.
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(4 * NP) hess_backward_seeds_kernel(HessArgs a) {
    constexpr int NW = NP / 16, NTH = 64 * NW, NP2 = NP * NP, CW = 16;
    __shared__ double Xr[NP * CW], Xi[NP * CW];
    __shared__ double red[NW][2][CW];
    __shared__ double dscale[HESS_MAX_L];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, N = a.s.N, N_T = a.s.N_T, L = a.s.L, npair = L * (L + 1) / 2;
    double *Am = a.ws + (size_t)k * 4 * NP2, *Bm = Am + 2 * NP2;
    const double *Hc = a.s.Hcf + (size_t)(a.s.hc_per_traj ? k : 0) * L * 2 * NP2;
    const double2 *fwk = a.s.fw + (size_t)k * (N_T + 1) * NP;
    const HessCol col = hess_column<1>(lc, L);
    d4 sr, si;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + 4 * r + lg;
        double2 x = make_double2(0., 0.);
        if (lc == 0 && row < N) x = a.s.target[(size_t)k * N + row];
        sr[r] = x.x; si[r] = x.y;
        Xr[row * CW + lc] = x.x; Xi[row * CW + lc] = x.y;
    }
    int maxo = HVP_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    for (int n = N_T - 1; n >= 0; --n) {
        double dt;
        const int msub = hvp_build_step<NP, NTH, true>(a.s, k, n, a.s.eps, Am, Bm, dt);
        if (tid < L) dscale[tid] = (a.s.shape ? a.s.shape[(size_t)tid * N_T + n] : 1.0) * dt;
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            const int na = hess_series_step<NP, 1>(a, Am, Hc, dscale, Xr, Xi, red, sr, si, col, wave, lane, maxo);
            if (na < 0) { failed = true; maxo = 1; } else terms += (unsigned long long)na;
            ++substeps;
        }
        if (lc >= 1 && lc <= L) {
            double2 *out = a.bv + (((size_t)k * N_T + n) * L + (lc - 1)) * NP;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[16 * wave + 4 * r + lg] = make_double2(sr[r], si[r]);
        }
        // <beta | Psi(t_n)>, <beta2 | Psi(t_n)>: rows of a lane, lane groups, then waves in index order
        {
            double dr = 0., di = 0.;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg;
                const double2 x = row < N ? fwk[(size_t)n * NP + row] : make_double2(0., 0.);
                dr += sr[r] * x.x + si[r] * x.y;
                di += sr[r] * x.y - si[r] * x.x;
            }
            dr += __shfl_xor(dr, 16, 64); di += __shfl_xor(di, 16, 64);
            dr += __shfl_xor(dr, 32, 64); di += __shfl_xor(di, 32, 64);
            if (lg == 0) { red[wave][0][lc] = dr; red[wave][1][lc] = di; }
        }
        __syncthreads();
        if (tid >= 1 && tid < 1 + L + npair) {
            double dr = 0., di = 0.;
            for (int w = 0; w < NW; ++w) { dr += red[w][0][tid]; di += red[w][1][tid]; }
            if (tid <= L) a.T[(size_t)k * N_T * L + (size_t)n * L + (tid - 1)] = make_double2(dr, di);
            else a.Sd[((size_t)k * N_T + n) * HESS_PAIRS + (tid - 1 - L)] = make_double2(dr, di);
        }
        // beta = beta2 = 0 for the next interval; theta carries on
        if (lc >= 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg;
                sr[r] = 0.; si[r] = 0.;
                Xr[row * CW + lc] = 0.; Xi[row * CW + lc] = 0.;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.s.flags[0], 16);
        a.stats[2 * (size_t)k] = terms;
        a.stats[2 * (size_t)k + 1] = substeps;
    }
}

// ---------------------------------------------------------------------------------------
// Fan: grid (ceil(P / 16), trajectories of the pass), NP / 16 waves.  Block b carries the columns q = 16 b .. 16 b + 15
// (q = m L + l', born at t_{m+1}) from the birth of its first column to the last grid point.
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(4 * NP) hess_fan_kernel(HessArgs a) {
    constexpr int NW = NP / 16, NTH = 64 * NW, NP2 = NP * NP, CW = 16;
    __shared__ double Xr[NP * CW], Xi[NP * CW];
    __shared__ double red[NW][2][CW];
    __shared__ double ovl[NW][HESS_MAX_L][2][CW];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, kk = blockIdx.y, k = a.k0 + kk, N_T = a.s.N_T, L = a.s.L, P = L * N_T;
    const size_t wg = (size_t)kk * gridDim.x + b;
    double *Am = a.ws + wg * 4 * NP2, *Bm = Am + 2 * NP2;
    double *strip = a.strip + (size_t)kk * P * P;
    const int q = 16 * b + lc, mq = q / L, lq = q - mq * L;   // the lane's column: born at t_{mq + 1}
    const bool exists = q < P;
    const double2 ck = hess_coef(a.s, k);
    HessCol col = hess_column<2>(lc, L);
    d4 sr = (d4){0., 0., 0., 0.}, si = (d4){0., 0., 0., 0.};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + 4 * r + lg;
        Xr[row * CW + lc] = 0.; Xi[row * CW + lc] = 0.;
    }
    int maxo = HVP_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    for (int n = (16 * b) / L + 1; n < N_T; ++n) {
        // the columns born at t_n
        if (exists && mq == n - 1) {
            const double2 *src = a.av + (((size_t)k * N_T + mq) * L + lq) * NP;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg;
                const double2 x = src[row];
                sr[r] = x.x; si[r] = x.y;
                Xr[row * CW + lc] = x.x; Xi[row * CW + lc] = x.y;
            }
        }
        // <beta_(n,l) | x_q> for every l: rows of a lane, lane groups, then waves in index order
#pragma unroll
        for (int l = 0; l < HESS_MAX_L; ++l) {
            if (l >= L) continue;
            const double2 *bt = a.bv + (((size_t)k * N_T + n) * L + l) * NP;
            double dr = 0., di = 0.;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double2 y = bt[16 * wave + 4 * r + lg];
                dr += y.x * sr[r] + y.y * si[r];
                di += y.x * si[r] - y.y * sr[r];
            }
            dr += __shfl_xor(dr, 16, 64); di += __shfl_xor(di, 16, 64);
            dr += __shfl_xor(dr, 32, 64); di += __shfl_xor(di, 32, 64);
            if (lg == 0) { ovl[wave][l][0][lc] = dr; ovl[wave][l][1][lc] = di; }
        }
        __syncthreads();   // the overlaps and the new columns are visible
        if (tid < 16 * L) {
            const int l = tid >> 4, c = tid & 15, qc = 16 * b + c;
            if (qc < P && qc / L < n) {
                double dr = 0., di = 0.;
                for (int w = 0; w < NW; ++w) { dr += ovl[w][l][0][c]; di += ovl[w][l][1][c]; }
                strip[((size_t)n * L + l) * P + qc] = ck.x * dr + ck.y * di;   // Re(conj(c_k) <beta | x>)
            }
        }
        if (n == N_T - 1) break;
        double dt;
        const int msub = hvp_build_step<NP, NTH, false>(a.s, k, n, a.s.eps, Am, Bm, dt);
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            const int na = hess_series_step<NP, 2>(a, Am, nullptr, nullptr, Xr, Xi, red, sr, si, col, wave, lane, maxo);
            if (na < 0) { failed = true; maxo = 1; } else terms += (unsigned long long)na;
            ++substeps;
        }
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.s.flags[0], 16);
        a.stats[2 * wg] = terms;
        a.stats[2 * wg + 1] = substeps;
    }
}

// ---------------------------------------------------------------------------------------
// acc += the strips of the pass, one trajectory after the other (ascending k whatever the pass size).  One thread per entry.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) hess_accumulate_kernel(HessArgs a, const int ntraj) {
    const int L = a.s.L, P = L * a.s.N_T;
    const size_t PP = (size_t)P * P, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= PP) return;
    const int r = (int)(idx / P), q = (int)(idx - (size_t)r * P);
    if (r / L <= q / L) return;
    double v = a.acc[idx];
    for (int kk = 0; kk < ntraj; ++kk) v += a.strip[(size_t)kk * PP + idx];
    a.acc[idx] = v;
}

// ---------------------------------------------------------------------------------------
// The lower triangle (interval-major r >= q): the fan's sum or the diagonal block, the boundary term, times -2; mirrored and
// mapped to p = l N_T + n.  Every sum over k in index order.  One thread per entry.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) hess_finish_kernel(HessArgs a) {
    const int L = a.s.L, N_T = a.s.N_T, P = L * N_T, K = a.s.K;
    const size_t PP = (size_t)P * P, idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= PP) return;
    const int r = (int)(idx / P), q = (int)(idx - (size_t)r * P);
    if (r < q) return;
    const int n = r / L, l = r - n * L, m = q / L, l2 = q - m * L;
    const double Kt = (double)a.s.K_total;
    double v;
    if (n > m) v = a.acc[idx];
    else {
        v = 0.;
        for (int k = 0; k < K; ++k) {
            const double2 c = hess_coef(a.s, k), s = a.Sd[((size_t)k * N_T + n) * HESS_PAIRS + l * (l + 1) / 2 + l2];
            v += c.x * s.x + c.y * s.y;
        }
    }
    // Re sum_k conj(d_q c_k) T_k,p
    double bnd = 0.;
    if (a.s.functional == 0) {
        double fr = 0., fi = 0.;
        for (int k = 0; k < K; ++k) {
            const double w = a.s.weights ? a.s.weights[k] : 1.0;
            const double2 t = a.T[(size_t)k * P + q];
            fr += w * t.x; fi += w * t.y;
        }
        for (int k = 0; k < K; ++k) {
            const double w = a.s.weights ? a.s.weights[k] : 1.0;
            const double2 t = a.T[(size_t)k * P + r];
            const double cr = w * fr / (Kt * Kt), ci = w * fi / (Kt * Kt);
            bnd += cr * t.x + ci * t.y;
        }
    } else if (a.s.functional == 1) {
        for (int k = 0; k < K; ++k) {
            const double w = a.s.weights ? a.s.weights[k] : 1.0;
            const double2 tq = a.T[(size_t)k * P + q], t = a.T[(size_t)k * P + r];
            const double cr = w * tq.x / Kt, ci = w * tq.y / Kt;
            bnd += cr * t.x + ci * t.y;
        }
    }
    const double out = -2.0 * (v + bnd);
    const size_t p = (size_t)l * N_T + n, pq = (size_t)l2 * N_T + m;
    a.H[p * P + pq] = out;
    a.H[pq * P + p] = out;
}
