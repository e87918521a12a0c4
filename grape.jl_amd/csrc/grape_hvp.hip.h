// grape_hvp.hip.h -- exact Hessian-vector products of J on the stored forward states (grape_hvp, N <= 64).
//
// A Newton-CG or trust-region solver needs H v at the current pulses, H = d^2 J / d eps^2.  The gradient is
//     G_nl = -2 Re sum_k <P_l | Psi_k(t_{n-1})>,   P_l = (DU_n[D_l])^dagger chi_k(t_n),
// so its derivative along a direction v is
//     (H v)_nl = -2 Re sum_k [ <P'_l | Psi_k(t_{n-1})> + <P_l | Psi'_k(t_{n-1})> ],
// where the prime is the derivative along v of everything that depends on the pulses: the states, the co-states, the
// propagators and the boundary coefficient of chi_k(T) = c_k tgt_k.  Per cell (k, n), with dt the (sub-)step,
//     A = -i H_kn dt,    D_l = -i s_ln dt H_l,    B = sum_l v_nl D_l,
// the power series of the exponential is differentiated term by term -- the block recursion of grape_lindblad.hip.h with
// one more level:
//   tangent forward sweep (hvp_forward_kernel), columns [u u']:
//       u_{a+1} = A u_a / (a+1),   u'_{a+1} = (A u'_a + B u_a) / (a+1);   u_0 = Psi_{n-1} (stored),  u'_0 = Psi'_{n-1}
//   boundary (hvp_boundary_kernel): f' = sum_k w_k tau'_k,  chi'_k(T) = c'_k tgt_k  (sm: w_k f' / K^2, ss: w_k tau'_k / K, re: 0)
//   backward sweep (hvp_backward_kernel), columns [c c' p_1..p_L p'_1..p'_L] under A^dagger:
//       c_{a+1}  = A^dagger c_a / (a+1)                       c'_{a+1} = (A^dagger c'_a + B^dagger c_a) / (a+1)
//       p_{a+1}  = (A^dagger p_a + D_l^dagger c_a) / (a+1)    p'_{a+1} = (A^dagger p'_a + B^dagger p_a + D_l^dagger c'_a) / (a+1)
//   The sums are chi_{n-1}, chi'_{n-1}, P_l, P'_l.  A long step is cut into m = ceil(beta_n dt_n / theta) sub-steps; all
//   chains carry over from one sub-step to the next (semigroup property of the exponential of the block generator).
//   A series stops when EVERY chain has ||term|| <= tol ||sum||, after at most HVP_MAX_ORDER terms (flag 16 otherwise).
//
// Layout on the chip.  One workgroup per (trajectory, direction), NP / 16 waves: wave w owns the rows [16 w, 16 w + 16) of
// every column.  The column block of the current terms lives in the LDS (planar, [row][column]); the running sums stay in
// the registers of the lane that owns the element.  A^dagger and B^dagger of the step are formed once per step in a
// per-workgroup workspace in device memory (it stays in the L2 / vector L1, as in the Lindblad kernels), the control
// operators are read where the handle keeps them.  Every product is a complex GEMM on v_mfma_f64_16x16x4_f64 tiles; the
// couplings between the chains are column selections of the B operand: the lane that owns column q of the result feeds
// column src(q) of the term block (or zero), so the products of one term accumulate into one tile.  2 + 2L columns are one
// column tile for L <= 7 and two for L = 8.  Everything runs in the balanced frame of the handle.
// Reductions have a fixed order (lane groups, then waves in index order): results are bitwise repeatable, and a direction
// never sees its neighbours -- its result does not depend on nv or on the launch groups.  No scratch memory.
#pragma once
#include "grape_kernels.hip.h"
#include "grape_series.hip.h"   // c_series_inv

#define HVP_MAX_ORDER 200

struct HvpArgs {
    const double *H0f;      // [K][2][NP*NP] planar row-major drift (balanced frame)
    const double *Hcf;      // [Kc][L][2][NP*NP] control operators
    const double *eps;      // [L][N_T] pulses of the last evaluation
    const double *shape;    // nullptr or [L][N_T]
    const double *dts;      // [N_T]
    const double *rb;       // [K] r0_k | [Kc][L] r_l: 2-norm estimates made at create time
    const double *V;        // [nd][L*N_T] directions of this launch group
    const double2 *fw;      // [K][N_T+1][NP] stored forward states Psi_k(t_n)
    const double2 *target;  // [K][N]
    const double *weights;  // nullptr or [K]
    const double2 *tau;     // [K] of the last evaluation
    const double *f;        // [2] sum_k w_k tau_k of the last evaluation
    double2 *dpsi;          // [nd][K][N_T+1][NP] Psi'_k(t_n)
    double2 *dtau;          // [nd][K] tau'_k
    double2 *dcoef;         // [nd][K] c'_k
    double2 *tg;            // [nd][K][L*N_T] per-trajectory terms of H v (input of grad_reduce_kernel)
    double *ws;             // [nd][K][2][2][NP*NP] step matrices of every workgroup
    int *flags;             // [0] |= 16: a series did not converge
    unsigned long long *stats;   // [2][nd*K][2]: series terms, (sub-)steps of the forward | backward workgroups
    double tol, theta;
    int K, K_total, L, N, N_T, functional, hc_per_traj;
};

__device__ __forceinline__ int hvp_substeps(const double beta, const double dt, const double theta) {
    const int m = (int)ceil(beta * dt / theta);
    return m < 1 ? 1 : (m > 4096 ? 4096 : m);   // (NaN: 1)
}

// acc += M X~ on one 16 x 16 tile.  M: planar in device memory; TR = false: M[row][k] at row * NP + k, TR = true: the
// conjugate transpose of what is stored (M[row][k] = conj(S[k][row])).  X~: column `col` of the term block in the LDS
// ([row][CW] planes), scaled by the complex lane constant (zr, zi) -- (1, 0) for a plain column, (0, 0) for none.
template <int NP, int CW, bool TR>
__device__ __forceinline__ void hvp_mac(d4 &cr, d4 &ci, const double *M, const int ti, const int lane, const double *Xr, const double *Xi,
                                        const int col, const double zr, const double zi) {
    constexpr int NP2 = NP * NP;
    const int lc = lane & 15, lg = lane >> 4;
    unsigned ao = TR ? (unsigned)(lg * NP + 16 * ti + lc) : (unsigned)((16 * ti + lc) * NP + lg);
    unsigned bo = (unsigned)(lg * CW + col);
#pragma unroll 4
    for (int ks = 0; ks < NP / 4; ++ks) {
        const double ar = M[ao], ai = TR ? -M[NP2 + ao] : M[NP2 + ao];
        const double xr = Xr[bo], xi = Xi[bo];
        const double br = zr * xr - zi * xi, bi = zr * xi + zi * xr;
        ao += TR ? 4 * NP : 4; bo += 4 * CW;
        cr = MFMA64(ar, br, cr);
        ci = MFMA64(ar, bi, ci);
        cr = MFMA64(-ai, bi, cr);
        ci = MFMA64(ai, br, ci);
    }
}

// the step matrices of interval n in the workspace, (sub-)step dt = dts[n] / m folded in; returns m (every thread the same).
//   ADJ = false: Am = A = -i dt H_kn,            Bm = B = -i dt sum_l v_nl s_ln H_l
//   ADJ = true : Am = A^dagger,                  Bm = B^dagger
template <int NP, int NTH, bool ADJ>
__device__ __forceinline__ int hvp_build_step(const HvpArgs &a, const int k, const int n, const double *v, double *Am, double *Bm, double &dt) {
    constexpr int NP2 = NP * NP;
    const int L = a.L, N_T = a.N_T, kc = a.hc_per_traj ? k : 0;
    const double *H0 = a.H0f + (size_t)k * 2 * NP2, *Hc = a.Hcf + (size_t)kc * L * 2 * NP2;
    double bound = a.rb[k];
    for (int l = 0; l < L; ++l)
        bound += fabs(a.eps[(size_t)l * N_T + n] * (a.shape ? a.shape[(size_t)l * N_T + n] : 1.0)) * a.rb[a.K + kc * L + l];
    const int m = hvp_substeps(bound, a.dts[n], a.theta);
    dt = a.dts[n] / (double)m;
    for (unsigned idx = threadIdx.x; idx < (unsigned)NP2; idx += NTH) {
        double hr = H0[idx], hi = H0[NP2 + idx], br = 0., bi = 0.;
        for (int l = 0; l < L; ++l) {
            const double s = a.shape ? a.shape[(size_t)l * N_T + n] : 1.0;
            const double e = a.eps[(size_t)l * N_T + n] * s, w = v[(size_t)l * N_T + n] * s;
            const double *hl = Hc + (size_t)l * 2 * NP2;
            const double cr = hl[idx], ci = hl[NP2 + idx];
            hr = fma(e, cr, hr); hi = fma(e, ci, hi);
            br = fma(w, cr, br); bi = fma(w, ci, bi);
        }
        // -i dt (x + i y) = dt y - i dt x;  its conjugate transpose: element (j, i) = dt y + i dt x
        if (ADJ) {
            const unsigned i = idx / NP, j = idx - i * NP, t = j * NP + i;
            Am[t] = dt * hi; Am[NP2 + t] = dt * hr;
            Bm[t] = dt * bi; Bm[NP2 + t] = dt * br;
        } else {
            Am[idx] = dt * hi; Am[NP2 + idx] = -dt * hr;
            Bm[idx] = dt * bi; Bm[NP2 + idx] = -dt * br;
        }
    }
    return m;
}

// What a lane does for column q of the block (the same for every row tile):
//   self : 1 if the column exists (A X, identity selection)
//   bsrc : the column B multiplies into q (bon = 1), or none (bon = 0)
//   dl   : the control whose D_l^dagger multiplies column dsrc into q, or -1
struct HvpCol {
    int bsrc, dsrc, dl;
    double self, bon;
};
template <bool BWD>
__device__ __forceinline__ HvpCol hvp_column(const int q, const int L) {
    HvpCol c;
    c.bsrc = 0; c.dsrc = 0; c.dl = -1; c.bon = 0.;
    if (!BWD) {                       // [u u']
        c.self = q < 2 ? 1. : 0.;
        if (q == 1) c.bon = 1.;
    } else {                          // [c c' p_1..p_L p'_1..p'_L]
        c.self = q < 2 + 2 * L ? 1. : 0.;
        if (q == 1) c.bon = 1.;
        else if (q >= 2 && q < 2 + L) c.dl = q - 2;
        else if (q >= 2 + L && q < 2 + 2 * L) { c.bon = 1.; c.bsrc = q - L; c.dl = q - 2 - L; c.dsrc = 1; }
    }
    return c;
}

// One (sub-)step of the block series on the column block in the LDS.  On entry X holds the start vectors and (sr, si) the
// same values; on exit (sr, si) hold the sums and X the sums as well (the start of the next sub-step).  Returns the
// number of terms, or -1 if the series has not converged.
template <int NP, int NCT, bool BWD>
__device__ __forceinline__ int hvp_series_step(const HvpArgs &a, const double *Am, const double *Bm, const double *Hc, const double *dscale,
                                               double *Xr, double *Xi, double (*red)[2][16 * NCT], d4 (&sr)[NCT], d4 (&si)[NCT],
                                               const HvpCol (&col)[NCT], const int wave, const int lane, const int maxo) {
    constexpr int CW = 16 * NCT, NW = NP / 16, NP2 = NP * NP;
    const int lc = lane & 15, lg = lane >> 4;
    const double tol2 = a.tol * a.tol;
    bool conv = false;
    int aord = 0;
    for (; aord < maxo && !conv; ++aord) {
        const double fac = c_series_inv[aord & 255];
        d4 tr[NCT], tim[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
            const int q = 16 * ct + lc;
            hvp_mac<NP, CW, false>(cr, ci, Am, wave, lane, Xr, Xi, q, col[ct].self, 0.);
            hvp_mac<NP, CW, false>(cr, ci, Bm, wave, lane, Xr, Xi, col[ct].bsrc, col[ct].bon, 0.);
            if (BWD) {
                for (int l = 0; l < a.L; ++l) {
                    // (uniform per wave: does this column tile hold p_l or p'_l at all?)
                    const int q0 = 2 + l, q1 = 2 + a.L + l;
                    if ((q0 >> 4) != ct && (q1 >> 4) != ct) continue;
                    // D_l^dagger = (-i s dt H_l)^dagger = (i s dt) H_l^dagger
                    hvp_mac<NP, CW, true>(cr, ci, Hc + (size_t)l * 2 * NP2, wave, lane, Xr, Xi, col[ct].dsrc, 0., col[ct].dl == l ? dscale[l] : 0.);
                }
            }
            double t2 = 0., s2 = 0.;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double ur = fac * cr[r], ui = fac * ci[r];
                tr[ct][r] = ur; tim[ct][r] = ui;
                sr[ct][r] += ur; si[ct][r] += ui;
                t2 += ur * ur + ui * ui;
                s2 += sr[ct][r] * sr[ct][r] + si[ct][r] * si[ct][r];
            }
            t2 += __shfl_xor(t2, 16, 64); s2 += __shfl_xor(s2, 16, 64);
            t2 += __shfl_xor(t2, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            if (lg == 0) { red[wave][0][q] = t2; red[wave][1][q] = s2; }
        }
        __syncthreads();   // every wave has read the old terms; the norms are visible
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = (16 * wave + 4 * r + lg) * CW + 16 * ct + lc;
                Xr[o] = tr[ct][r]; Xi[o] = tim[ct][r];
            }
        bool ok = true;
        if (lane < CW) {
            double t2 = 0., s2 = 0.;
#pragma unroll
            for (int w = 0; w < NW; ++w) { t2 += red[w][0][lane]; s2 += red[w][1][lane]; }
            ok = t2 <= tol2 * s2;
        }
        conv = __ballot(!ok) == 0ull;
        __syncthreads();   // the new terms are visible; the norms have been read
    }
    // the sums are the start vectors of the next (sub-)step
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = (16 * wave + 4 * r + lg) * CW + 16 * ct + lc;
            Xr[o] = sr[ct][r]; Xi[o] = si[ct][r];
        }
    __syncthreads();
    return conv ? aord : -1;
}

// ---------------------------------------------------------------------------------------
// Tangent forward sweep: grid (K, directions), NP / 16 waves.  Stores Psi'_k(t_n) and tau'_k = <tgt_k | Psi'_k(T)>.
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(4 * NP) hvp_forward_kernel(HvpArgs a) {
    constexpr int NW = NP / 16, NTH = 64 * NW, NP2 = NP * NP, CW = 16;
    __shared__ double Xr[NP * CW], Xi[NP * CW];
    __shared__ double red[NW][2][CW];
    __shared__ double part[NW][2];
    const int tid = threadIdx.x, lane = tid & 63, lc = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, j = blockIdx.y, N = a.N, N_T = a.N_T;
    const size_t wg = (size_t)j * a.K + k;
    double *Am = a.ws + wg * 4 * NP2, *Bm = Am + 2 * NP2;
    const double *v = a.V + (size_t)j * a.L * N_T;
    const double2 *fwk = a.fw + (size_t)k * (N_T + 1) * NP;
    double2 *dps = a.dpsi + wg * (size_t)(N_T + 1) * NP;
    HvpCol col[1];
    col[0] = hvp_column<false>(lc, a.L);

    d4 sr[1], si[1];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + 4 * r + lg;
        double2 x = make_double2(0., 0.);
        if (lc == 0 && row < N) x = fwk[row];
        sr[0][r] = x.x; si[0][r] = x.y;
        Xr[row * CW + lc] = x.x; Xi[row * CW + lc] = x.y;
        if (lc == 1) dps[row] = make_double2(0., 0.);   // Psi'(t_0) = 0
    }
    int maxo = HVP_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    for (int n = 0; n < N_T; ++n) {
        double dt;
        const int msub = hvp_build_step<NP, NTH, false>(a, k, n, v, Am, Bm, dt);
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            const int na = hvp_series_step<NP, 1, false>(a, Am, Bm, nullptr, nullptr, Xr, Xi, red, sr, si, col, wave, lane, maxo);
            if (na < 0) { failed = true; maxo = 1; } else terms += (unsigned long long)na;
            ++substeps;
        }
        // Psi'(t_{n+1}) out; u restarts from the stored Psi(t_{n+1})
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * wave + 4 * r + lg;
            if (lc == 1) dps[(size_t)(n + 1) * NP + row] = make_double2(sr[0][r], si[0][r]);
            if (lc == 0) {
                const double2 x = row < N ? fwk[(size_t)(n + 1) * NP + row] : make_double2(0., 0.);
                sr[0][r] = x.x; si[0][r] = x.y;
                Xr[row * CW] = x.x; Xi[row * CW] = x.y;
            }
        }
        __syncthreads();
    }
    {   // tau'_k = <tgt_k | Psi'_k(T)>
        double pr = 0., pi = 0.;
        if (lc == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg;
                if (row < N) {
                    const double2 t = a.target[(size_t)k * N + row];
                    pr += t.x * sr[0][r] + t.y * si[0][r];
                    pi += t.x * si[0][r] - t.y * sr[0][r];
                }
            }
        }
        pr = wave_sum(pr); pi = wave_sum(pi);
        if (lane == 0) { part[wave][0] = pr; part[wave][1] = pi; }
        __syncthreads();
        if (tid == 0) {
            pr = 0.; pi = 0.;
            for (int w = 0; w < NW; ++w) { pr += part[w][0]; pi += part[w][1]; }
            a.dtau[wg] = make_double2(pr, pi);
            if (failed) atomicOr(&a.flags[0], 16);
            a.stats[2 * wg] = terms;
            a.stats[2 * wg + 1] = substeps;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Boundary: f' = sum_k w_k tau'_k in a fixed order and c'_k of chi'_k(T) = c'_k tgt_k.  Grid (directions), one wave.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) hvp_boundary_kernel(HvpArgs a) {
    const int j = blockIdx.x, lane = threadIdx.x, K = a.K;
    const double2 *dt = a.dtau + (size_t)j * K;
    double fr = 0., fi = 0.;
    for (int k = lane; k < K; k += 64) {
        const double w = a.weights ? a.weights[k] : 1.0;
        fr += w * dt[k].x; fi += w * dt[k].y;
    }
    fr = wave_sum(fr); fi = wave_sum(fi);
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
// Backward sweep: grid (K, directions), NP / 16 waves, NCT column tiles (2 + 2L columns).
// ---------------------------------------------------------------------------------------
template <int NP, int NCT>
__global__ void __launch_bounds__(4 * NP) hvp_backward_kernel(HvpArgs a) {
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

    // chi_k(T) = c_k tgt_k (include/grape_hip.h), chi'_k(T) = c'_k tgt_k; p = p' = 0
    d4 sr[NCT], si[NCT];
    {
        const double w = a.weights ? a.weights[k] : 1.0, Kt = (double)a.K_total;
        double c0r, c0i;
        if (a.functional == 0) { c0r = w * a.f[0] / (Kt * Kt); c0i = w * a.f[1] / (Kt * Kt); }
        else if (a.functional == 1) { const double2 t = a.tau[k]; c0r = w * t.x / Kt; c0i = w * t.y / Kt; }
        else { c0r = w / (2.0 * Kt); c0i = 0.; }
        const double2 c1 = a.dcoef[wg];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * wave + 4 * r + lg, q = 16 * ct + lc;
                double xr = 0., xi = 0.;
                if (q < 2 && row < N) {
                    const double2 t = a.target[(size_t)k * N + row];
                    const double cr = q == 0 ? c0r : c1.x, ci = q == 0 ? c0i : c1.y;
                    xr = cr * t.x - ci * t.y; xi = cr * t.y + ci * t.x;
                }
                sr[ct][r] = xr; si[ct][r] = xi;
                Xr[row * CW + q] = xr; Xi[row * CW + q] = xi;
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
