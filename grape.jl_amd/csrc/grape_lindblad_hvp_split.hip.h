// grape_lindblad_hvp_split.hip.h -- the Hessian-vector product of grape_lindblad_hvp.hip.h cut at its one cross-trajectory
// dependency (grape_open_hvp_forward / grape_open_hvp_backward / grape_open_hvp_backward_chi).
//
// grape_open_hvp runs tangent forward sweep, boundary, backward sweep in one call.  Between the sweeps sits the only quantity
// that couples the trajectories, f' = sum_k w_k tau'_k, and the only place where the functional enters, the boundary
// chi_k(T) = c_k sigma_k, chi'_k(T) = c'_k sigma_k.  A trajectory shard (K < K_total) has to all-reduce f' on the host, a
// caller's functional has to supply chi and chi' itself.  So:
//   forward half : lind_hvp_forward_kernel as it is, then lind_hvp_partial_sum_kernel: sum_k w_k tau'_k of THIS handle's
//                  trajectories; lind_hvp_final_tangent_kernel packs rho'_k(T) for one copy to the host
//   built-in     : lind_hvp_coef_total_kernel fills c'_k from the all-reduced f', then lind_hvp_backward_kernel as it is (its
//                  f is a pointer: it reads the all-reduced f the caller passed)
//   caller's chi : lind_hvp_backward_chi_kernel -- lind_hvp_backward_kernel restated with C[0], sum C loaded from
//                  chi [K][2][NP^2] and C'[0], sum C' from dchi [nd][K][2][NP^2] (planar row-major, zero padded) instead of
//                  formed as c sigma.
// The two small kernels repeat the loops and expressions of lind_hvp_boundary_kernel, so that on an unsharded handle the two
// halves give the bits of grape_open_hvp.  The restated sweep shares lind_build_generator, lind_hvp_build_direction,
// lind_hvp_tile, lind_left_products, lind_mac, lind_apply_tile and lind_hvp_commit with the original (same workspace layout
// with the run-time chain index, same red[2][8][NW], same barriers, fixed-order reductions, no atomics on floating point, no
// scratch); the original is not routed through a shared body.
#pragma once
#include "grape_lindblad_hvp.hip.h"

// ---------------------------------------------------------------------------------------
// sum_k w_k tau'_k over the trajectories of this handle: grid (directions), one wave; psums [nd][2]
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) lind_hvp_partial_sum_kernel(LindHvpArgs q, double *psums) {
    const int jd = blockIdx.x, lane = threadIdx.x, K = q.a.K;
    const double2 *dt = q.dtau + (size_t)jd * K;
    double fr = 0., fi = 0.;
    for (int k = lane; k < K; k += 64) {
        const double w = q.a.weights ? q.a.weights[k] : 1.0;
        fr += w * dt[k].x; fi += w * dt[k].y;
    }
    fr = wave_sum(fr); fi = wave_sum(fi);
    if (lane == 0) { psums[2 * jd] = fr; psums[2 * jd + 1] = fi; }
}

// ---------------------------------------------------------------------------------------
// c'_k of chi'_k(T) = c'_k sigma_k from the all-reduced f' (df_total [nd][2]): grid (directions), one wave
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) lind_hvp_coef_total_kernel(LindHvpArgs q, const double *df_total) {
    const int jd = blockIdx.x, lane = threadIdx.x, K = q.a.K;
    const double2 *dt = q.dtau + (size_t)jd * K;
    const double fr = df_total[2 * jd], fi = df_total[2 * jd + 1];
    const double Kt = (double)q.a.K_total;
    for (int k = lane; k < K; k += 64) {
        const double w = q.a.weights ? q.a.weights[k] : 1.0;
        double2 c = make_double2(0., 0.);
        if (q.a.functional == 0) c = make_double2(w * fr / (Kt * Kt), w * fi / (Kt * Kt));
        else if (q.a.functional == 1) c = make_double2(w * dt[k].x / Kt, w * dt[k].y / Kt);
        q.dcoef[(size_t)jd * K + k] = c;
    }
}

// ---------------------------------------------------------------------------------------
// rho'_k(T) of every (direction, trajectory), packed for ONE copy to the host on the handle's stream: out [nd K][2][NP^2]
// (planar row-major, as stored).  Grid (nd K), 256 threads.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lind_hvp_final_tangent_kernel(LindHvpArgs q, int m2, double *out) {
    const size_t wg = blockIdx.x;
    const double *src = q.dstore + (wg * (size_t)(q.a.N_T + 1) + (size_t)q.a.N_T) * (size_t)m2;
    for (int i = threadIdx.x; i < m2; i += 256) out[wg * (size_t)m2 + i] = src[i];
}

// ---------------------------------------------------------------------------------------
// Backward sweep from the caller's boundary: grid (K, L, directions), one control per workgroup, waves as LindBwd<NP>.
// chi [K][2][NP^2], dchi [nd][K][2][NP^2]: planar row-major, rows and columns N..NP-1 zero.  Reads neither targets, weights,
// tau, f nor the functional.
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(LindBwd<NP>::NTH) lind_hvp_backward_chi_kernel(LindHvpArgs q, const double *chi, const double *dchi) {
    constexpr int TPW = LindBwd<NP>::TPW, NW = LindBwd<NP>::NW, NTH = LindBwd<NP>::NTH, NP2 = NP * NP;
    __shared__ double red[2][8][NW];
    const LindArgs &a = q.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, l = blockIdx.y, jd = blockIdx.z;
    const int J = a.J, N_T = a.N_T, L = a.L;
    const size_t wd = (size_t)jd * a.K + k, wg = ((size_t)jd * L + l) * a.K + k;
    double *ws = q.ws + wg * (16 + 4 * J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *B = ws + 4 * NP2, *Bd = ws + 6 * NP2;
    double *Cb = ws + 8 * NP2, *Cpb = ws + 12 * NP2, *Pb = ws + 16 * NP2, *Ppb = ws + 20 * NP2;
    lind_gd *Cs = lind_uniform(ws + 24 * NP2), *Cps = lind_uniform(ws + 26 * NP2), *Ps = lind_uniform(ws + 28 * NP2),
            *Pps = lind_uniform(ws + 30 * NP2);
    double *Tc = ws + 32 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    const double *Dl = a.Dc + ((size_t)(a.hc_per_traj ? k : 0) * L + l) * 4 * NP2, *Dld = Dl + 2 * NP2;
    const double *v = q.V + (size_t)jd * L * N_T;
    const double *st = a.store + (size_t)k * (N_T + 1) * 2 * NP2;
    const double *ds = q.dstore + wd * (size_t)(N_T + 1) * 2 * NP2;
    int par = 0;

    {   // chi_k(T), chi'_k(T) as the caller gave them
        const lind_gd *xg = lind_uniform(chi + (size_t)k * 2 * NP2), *xpg = lind_uniform(dchi + wd * 2 * NP2);
        lind_gd *C0 = lind_uniform(Cb), *Cp0 = lind_uniform(Cpb);
        for (int t = 0; t < TPW; ++t) {
            const LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double vr = xg[g.o[r]], vi = xg[NP2 + g.o[r]];
                const double wr = xpg[g.o[r]], wi = xpg[NP2 + g.o[r]];
                Cs[g.o[r]] = vr; Cs[NP2 + g.o[r]] = vi; C0[g.o[r]] = vr; C0[NP2 + g.o[r]] = vi;
                Cps[g.o[r]] = wr; Cps[NP2 + g.o[r]] = wi; Cp0[g.o[r]] = wr; Cp0[NP2 + g.o[r]] = wi;
            }
        }
    }
    int cur = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int step = 0; step < N_T; ++step) {
        const int n = N_T - 1 - step;
        const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
        lind_hvp_build_direction<NP, NTH>(a, v, k, n, B, Bd);
        const int msub = lind_substeps(beta, a.dts[n], a.theta);
        const double dt = a.dts[n] / (double)msub;
        const double sh = a.shape ? a.shape[(size_t)l * N_T + n] : 1.0;
        {
            lind_gd *P0 = lind_uniform(Pb + (size_t)cur * 2 * NP2), *Pp0 = lind_uniform(Ppb + (size_t)cur * 2 * NP2);
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    P0[g.o[r]] = 0.; P0[NP2 + g.o[r]] = 0.; Ps[g.o[r]] = 0.; Ps[NP2 + g.o[r]] = 0.;
                    Pp0[g.o[r]] = 0.; Pp0[NP2 + g.o[r]] = 0.; Pps[g.o[r]] = 0.; Pps[NP2 + g.o[r]] = 0.;
                }
            }
        }
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            bool conv = false;
            int aord = 0;
            for (; aord < maxo && !conv; ++aord) {
                // chain ch is a run-time index, as in lind_hvp_backward_kernel: one chain's operands are live at a time
                const double *Xb = Cb + (size_t)cur * 2 * NP2;
                double *Yb = Cb + (size_t)(cur ^ 1) * 2 * NP2;
                if (J > 0) {
#pragma unroll 1
                    for (int ch = 0; ch < 4; ++ch)
#pragma unroll 1
                        for (int t = 0; t < TPW; ++t) {
                            LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
                            lind_left_products<NP>(Tc + (size_t)ch * J * 2 * NP2, A + 2 * NP2, Xb + (size_t)ch * 4 * NP2, J, g.aoff, g.boff, g.o);
                        }
                    __syncthreads();
                }
                const double fac = dt * c_series_inv[aord & 255];
#pragma unroll 1
                for (int ch = 0; ch < 4; ++ch) {
                    // c: L^dagger c | c': B^dagger c + L^dagger c' | p: D_l^dagger c + L^dagger p | p': D_l^dagger c' + B^dagger p + L^dagger p'
                    const double *Xd = Xb + (size_t)(ch == 2 ? 0 : 1) * 4 * NP2;   // what D_l^dagger acts on (ch >= 2)
                    const double *Xv = Xb + (size_t)(ch == 1 ? 0 : 2) * 4 * NP2;   // what B^dagger acts on (ch odd)
                    const double *X = Xb + (size_t)ch * 4 * NP2, *Tx = Tc + (size_t)ch * J * 2 * NP2;
                    lind_gd *Y = lind_uniform(Yb + (size_t)ch * 4 * NP2), *S = lind_uniform(Cs + (size_t)ch * 2 * NP2);
                    double t2 = 0., s2 = 0.;
#pragma unroll 1
                    for (int t = 0; t < TPW; ++t) {
                        LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
                        d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                        if (ch >= 2) {
                            lind_mac<NP>(cr, ci, Dld, Xd, g.aoff, g.boff);
                            lind_mac<NP>(cr, ci, Xd, Dl, g.aoff, g.boff);
#pragma unroll
                            for (int r = 0; r < 4; ++r) { cr[r] *= sh; ci[r] *= sh; }
                        }
                        if (ch & 1) {
                            lind_mac<NP>(cr, ci, Bd, Xv, g.aoff, g.boff);
                            lind_mac<NP>(cr, ci, Xv, B, g.aoff, g.boff);
                        }
                        lind_apply_tile<NP>(cr, ci, Md, M, X, Tx, A, J, g.aoff, g.boff);
                        lind_hvp_commit<NP>(cr, ci, fac, Y, S, g.o, t2, s2);
                    }
                    t2 = wave_sum(t2); s2 = wave_sum(s2);
                    if (lane == 0) { red[par][2 * ch][wave] = t2; red[par][2 * ch + 1][wave] = s2; }
                }
                __syncthreads();
                conv = true;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double t2 = 0., s2 = 0.;
#pragma unroll
                    for (int w = 0; w < NW; ++w) { t2 += red[par][2 * c][w]; s2 += red[par][2 * c + 1][w]; }
                    conv = conv && t2 <= tol2 * s2;
                }
                par ^= 1; cur ^= 1;
            }
            if (!conv) { failed = true; maxo = 1; }
            terms += (unsigned long long)aord;
            ++substeps;
            // the chains of the next (sub-)step start from the sums: the buffers of the last terms are no longer read by anyone
            lind_gd *Cx = lind_uniform(Cb + (size_t)cur * 2 * NP2), *Cpx = lind_uniform(Cpb + (size_t)cur * 2 * NP2);
            lind_gd *Px = lind_uniform(Pb + (size_t)cur * 2 * NP2), *Ppx = lind_uniform(Ppb + (size_t)cur * 2 * NP2);
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    Cx[g.o[r]] = Cs[g.o[r]]; Cx[NP2 + g.o[r]] = Cs[NP2 + g.o[r]];
                    Cpx[g.o[r]] = Cps[g.o[r]]; Cpx[NP2 + g.o[r]] = Cps[NP2 + g.o[r]];
                    Px[g.o[r]] = Ps[g.o[r]]; Px[NP2 + g.o[r]] = Ps[NP2 + g.o[r]];
                    Ppx[g.o[r]] = Pps[g.o[r]]; Ppx[NP2 + g.o[r]] = Pps[NP2 + g.o[r]];
                }
            }
            __syncthreads();
        }
        {   // the term of (H v)_nl of this trajectory: <<P'_l | rho_k(t_n)>> + <<P_l | rho'_k(t_n)>>
            const lind_gd *x = lind_uniform(st + (size_t)n * 2 * NP2), *y = lind_uniform(ds + (size_t)n * 2 * NP2);
            double dr = 0., di = 0.;
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double xr = x[g.o[r]], xi = x[NP2 + g.o[r]], ppr = Pps[g.o[r]], ppi = Pps[NP2 + g.o[r]];
                    const double yr = y[g.o[r]], yi = y[NP2 + g.o[r]], pr = Ps[g.o[r]], pi = Ps[NP2 + g.o[r]];
                    dr += ppr * xr + ppi * xi;
                    di += ppr * xi - ppi * xr;
                    dr += pr * yr + pi * yi;
                    di += pr * yi - pi * yr;
                }
            }
            dr = wave_sum(dr); di = wave_sum(di);
            if (lane == 0) { red[par][0][wave] = dr; red[par][1][wave] = di; }
            __syncthreads();
            if (tid == 0) {
                dr = 0.; di = 0.;
                for (int w = 0; w < NW; ++w) { dr += red[par][0][w]; di += red[par][1][w]; }
                q.tg[(wd * L + l) * N_T + n] = make_double2(dr, di);
            }
            par ^= 1;
        }
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        const size_t sb = (size_t)q.nd * a.K + wg;
        q.stats[2 * sb] = terms;
        q.stats[2 * sb + 1] = substeps;
    }
}
