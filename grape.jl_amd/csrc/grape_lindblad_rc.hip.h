// grape_lindblad_rc.hip.h -- state running costs on open-system handles (grape_open_set_running_cost, grape_open_backward_xi,
// DESIGN.md 19).
//
// The reference's running cost J_b = sum_k sum_n wq_n g_b(rho_k(t_n)) (optimize.jl:727-750) enters the backward sweep as an
// inhomogeneity (optimize.jl:856-866, 897-908): with dg_b = -2 Re <<xi | d rho>>
//     chi_k(T)   = c_k sigma_k (or the caller's) + lambda_b wq_{N_T} xi_k(T),   rho_k = ||chi_k(T)||_F,   chi_k(T) /= rho_k
//     chi_k(t_n) += (lambda_b wq_n / rho_k) xi_k(t_n)      after interval n has been stepped back and tau_grads[k][l][n] formed,
//                                                          for n > 0 (chi_k(t_0) is nobody's input)
// The p chain restarts from zero on every interval and never sees the term; a cut interval gets it once, behind its last
// sub-step.  The built-in family is g_b(rho) = Re tr(D rho) = Re <<D^dagger | rho>>, whose xi is the constant Xi_k = -D_k^dagger / 2;
// a caller's xi is [K][N_T + 1] matrices.  Both are read through ONE pointer with two strides (k: 0 for a shared D; n: 0 for
// the constant), planar row-major NP x NP, zero padded, like every other matrix of grape_lindblad.hip.h.
//
// lind_backward_rc_kernel repeats the text of lind_backward_kernel with the two additions instead of sharing a body with it,
// for the reason grape_lindblad_batch.hip.h gives: the ordinary instantiations are to stay what they are, instruction for
// instruction, and a handle without a running cost launches them.  A change to the arithmetic of one file belongs in the
// other.  The additions are element-wise on the lane's own elements of the running sum (Cs) and of the current c buffer, so
// the barrier that follows the zeroing of the p chain at the top of the next interval is the one the next series needs;
// every workgroup (k, l) adds the same numbers in the same order, so rho_k and the chi chain stay identical across l.
// No floating-point atomics, no scratch memory, 1 KB of LDS; results are bitwise repeatable.
#pragma once
#include "grape_lindblad.hip.h"

struct LindRcArgs {
    const double *xi;      // xi_k(t_n) at xi + k stride_k + n stride_n: [2][NP*NP] planar
    size_t stride_k;       // doubles: 0 (shared D), 2 NP^2 (D per trajectory) or (N_T + 1) 2 NP^2 (the caller's xi)
    size_t stride_n;       // doubles: 0 (the built-in constant) or 2 NP^2 (the caller's xi)
    const double *wq;      // [N_T+1] trapezoid weights
    double lambda_b;
};

template <int NP>
__global__ void __launch_bounds__(LindBwd<NP>::NTH) lind_backward_rc_kernel(LindArgs a, LindRcArgs rc) {
    constexpr int TPW = LindBwd<NP>::TPW, NW = LindBwd<NP>::NW, NTH = LindBwd<NP>::NTH, NP2 = NP * NP;
    __shared__ double red[2][4][NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, l = blockIdx.y;
    const int J = a.J, N_T = a.N_T, L = a.L;
    const size_t wg = (size_t)l * a.K + k;
    double *ws = a.ws + wg * (8 + 2 * J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *Cb = ws + 4 * NP2, *Pb = ws + 8 * NP2, *Tc = ws + 16 * NP2, *Tp = Tc + (size_t)J * 2 * NP2;
    lind_gd *Cs = lind_uniform(ws + 12 * NP2), *Ps = lind_uniform(ws + 14 * NP2);
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    const double *Dl = a.Dc + ((size_t)(a.hc_per_traj ? k : 0) * L + l) * 4 * NP2, *Dld = Dl + 2 * NP2;
    const double *st = a.store + (size_t)k * (N_T + 1) * 2 * NP2;
    const double *xik = rc.xi + (size_t)k * rc.stride_k;
    int par = 0;

    // chi_k(T) = c_k sigma_k of the built-in functionals (include/grape_hip.h) or the caller's, plus lambda_b wq_{N_T} xi_k(T);
    // rho_k = ||chi_k||_F; chi_k /= rho_k
    double rho_k;   // (every workgroup (k, l) forms it in the same order)
    {
        double cfr = 0., cfi = 0.;
        const double *src = a.chi_in ? a.chi_in : a.target;
        if (a.chi_in) { cfr = 1.0; }
        else {
            const double w = a.weights ? a.weights[k] : 1.0, Kt = (double)a.K_total;
            if (a.functional == 0) { cfr = w * a.f[0] / (Kt * Kt); cfi = w * a.f[1] / (Kt * Kt); }
            else if (a.functional == 1) { const double2 t = a.tau[k]; cfr = w * t.x / Kt; cfi = w * t.y / Kt; }
            else { cfr = w / (2.0 * Kt); }
        }
        const lind_gd *sg = lind_uniform(src + (size_t)k * 2 * NP2);
        const lind_gd *xT = lind_uniform(xik + (size_t)N_T * rc.stride_n);
        const double cT = rc.lambda_b * rc.wq[N_T];
        lind_gd *C0 = lind_uniform(Cb);
        double n2 = 0.;
        for (int t = 0; t < TPW; ++t) {
            const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double tr = sg[g.o[r]], tim = sg[NP2 + g.o[r]];
                const double vr = (cfr * tr - cfi * tim) + cT * xT[g.o[r]], vi = (cfr * tim + cfi * tr) + cT * xT[NP2 + g.o[r]];
                n2 += vr * vr + vi * vi;
                Cs[g.o[r]] = vr; Cs[NP2 + g.o[r]] = vi;
            }
        }
        n2 = wave_sum(n2);
        if (lane == 0) red[par][0][wave] = n2;
        __syncthreads();
        n2 = 0.;
#pragma unroll
        for (int w = 0; w < NW; ++w) n2 += red[par][0][w];
        par ^= 1;
        rho_k = sqrt(n2);
        if (tid == 0 && l == 0) {
            a.rho[k] = rho_k;
            if (!(rho_k >= a.chi_min_norm)) atomicOr(&a.flags[0], 2);
        }
        const double ir = rho_k > 0. ? 1.0 / rho_k : 0.;
        for (int t = 0; t < TPW; ++t) {
            const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double vr = Cs[g.o[r]] * ir, vi = Cs[NP2 + g.o[r]] * ir;
                Cs[g.o[r]] = vr; Cs[NP2 + g.o[r]] = vi;
                C0[g.o[r]] = vr; C0[NP2 + g.o[r]] = vi;
            }
        }
    }
    const double irho = rho_k > 0. ? 1.0 / rho_k : 0.;
    int cur = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int step = 0; step < N_T; ++step) {
        const int n = N_T - 1 - step;
        const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
        const int msub = lind_substeps(beta, a.dts[n], a.theta);
        const double dt = a.dts[n] / (double)msub;
        const double sh = a.shape ? a.shape[(size_t)l * N_T + n] : 1.0;
        {
            lind_gd *P0 = lind_uniform(Pb + (size_t)cur * 2 * NP2);
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) { P0[g.o[r]] = 0.; P0[NP2 + g.o[r]] = 0.; Ps[g.o[r]] = 0.; Ps[NP2 + g.o[r]] = 0.; }
            }
        }
        __syncthreads();   // (also publishes the inhomogeneity the previous interval added to the current c buffer)
        for (int sub = 0; sub < msub; ++sub) {
            bool conv = false;
            int aord = 0;
            for (; aord < maxo && !conv; ++aord) {
                const double *Cx = Cb + (size_t)cur * 2 * NP2, *Px = Pb + (size_t)cur * 2 * NP2;
                lind_gd *Cy = lind_uniform(Cb + (size_t)(cur ^ 1) * 2 * NP2), *Py = lind_uniform(Pb + (size_t)(cur ^ 1) * 2 * NP2);
                if (J > 0) {
                    for (int t = 0; t < TPW; ++t) {
                        const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
                        lind_left_products<NP>(Tc, A + 2 * NP2, Cx, J, g.aoff, g.boff, g.o);
                        lind_left_products<NP>(Tp, A + 2 * NP2, Px, J, g.aoff, g.boff, g.o);
                    }
                    __syncthreads();
                }
                const double fac = dt * c_series_inv[aord & 255];
                double tc2 = 0., sc2 = 0., tp2 = 0., sp2 = 0.;
                for (int t = 0; t < TPW; ++t) {
                    const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
                    {
                        d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                        lind_apply_tile<NP>(cr, ci, Md, M, Cx, Tc, A, J, g.aoff, g.boff);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double ur = fac * cr[r], ui = fac * ci[r];
                            Cy[g.o[r]] = ur; Cy[NP2 + g.o[r]] = ui;
                            const double vr = Cs[g.o[r]] + ur, vi = Cs[NP2 + g.o[r]] + ui;
                            Cs[g.o[r]] = vr; Cs[NP2 + g.o[r]] = vi;
                            tc2 += ur * ur + ui * ui;
                            sc2 += vr * vr + vi * vi;
                        }
                    }
                    {
                        d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                        lind_mac<NP>(cr, ci, Dld, Cx, g.aoff, g.boff);
                        lind_mac<NP>(cr, ci, Cx, Dl, g.aoff, g.boff);
#pragma unroll
                        for (int r = 0; r < 4; ++r) { cr[r] *= sh; ci[r] *= sh; }
                        lind_apply_tile<NP>(cr, ci, Md, M, Px, Tp, A, J, g.aoff, g.boff);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double ur = fac * cr[r], ui = fac * ci[r];
                            Py[g.o[r]] = ur; Py[NP2 + g.o[r]] = ui;
                            const double vr = Ps[g.o[r]] + ur, vi = Ps[NP2 + g.o[r]] + ui;
                            Ps[g.o[r]] = vr; Ps[NP2 + g.o[r]] = vi;
                            tp2 += ur * ur + ui * ui;
                            sp2 += vr * vr + vi * vi;
                        }
                    }
                }
                tc2 = wave_sum(tc2); sc2 = wave_sum(sc2); tp2 = wave_sum(tp2); sp2 = wave_sum(sp2);
                if (lane == 0) { red[par][0][wave] = tc2; red[par][1][wave] = sc2; red[par][2][wave] = tp2; red[par][3][wave] = sp2; }
                __syncthreads();
                tc2 = 0.; sc2 = 0.; tp2 = 0.; sp2 = 0.;
#pragma unroll
                for (int w = 0; w < NW; ++w) { tc2 += red[par][0][w]; sc2 += red[par][1][w]; tp2 += red[par][2][w]; sp2 += red[par][3][w]; }
                par ^= 1; cur ^= 1;
                conv = tc2 <= tol2 * sc2 && tp2 <= tol2 * sp2;
            }
            if (!conv) { failed = true; maxo = 1; }
            terms += (unsigned long long)aord;
            ++substeps;
            // (c, p) of the next (sub-)step: the buffers of the last terms are no longer read by anyone
            lind_gd *Cx = lind_uniform(Cb + (size_t)cur * 2 * NP2), *Px = lind_uniform(Pb + (size_t)cur * 2 * NP2);
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    Cx[g.o[r]] = Cs[g.o[r]]; Cx[NP2 + g.o[r]] = Cs[NP2 + g.o[r]];
                    Px[g.o[r]] = Ps[g.o[r]]; Px[NP2 + g.o[r]] = Ps[NP2 + g.o[r]];
                }
            }
            __syncthreads();
        }
        {   // tau_grads[k][l][n] = rho_k <<sum_a p_a | rho_k(t_n)>>   (optimize.jl:894)
            const lind_gd *x = lind_uniform(st + (size_t)n * 2 * NP2);
            double dr = 0., di = 0.;
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double xr = x[g.o[r]], xi = x[NP2 + g.o[r]], pr = Ps[g.o[r]], pi = Ps[NP2 + g.o[r]];
                    dr += pr * xr + pi * xi;
                    di += pr * xi - pi * xr;
                }
            }
            dr = wave_sum(dr); di = wave_sum(di);
            if (lane == 0) { red[par][0][wave] = dr; red[par][1][wave] = di; }
            __syncthreads();
            if (tid == 0) {
                dr = 0.; di = 0.;
                for (int w = 0; w < NW; ++w) { dr += red[par][0][w]; di += red[par][1][w]; }
                a.tg[((size_t)k * L + l) * N_T + n] = make_double2(rho_k * dr, rho_k * di);
            }
            par ^= 1;
        }
        if (n > 0) {   // chi_k(t_n) += (lambda_b wq_n / rho_k) xi_k(t_n): the running sum and u_0 of the next series (optimize.jl:897-908)
            const lind_gd *xn = lind_uniform(xik + (size_t)n * rc.stride_n);
            lind_gd *Cx = lind_uniform(Cb + (size_t)cur * 2 * NP2);
            const double c = rc.lambda_b * rc.wq[n] * irho;
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double vr = Cs[g.o[r]] + c * xn[g.o[r]], vi = Cs[NP2 + g.o[r]] + c * xn[NP2 + g.o[r]];
                    Cs[g.o[r]] = vr; Cs[NP2 + g.o[r]] = vi;
                    Cx[g.o[r]] = vr; Cx[NP2 + g.o[r]] = vi;
                }
            }
        }
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        a.stats[2 * ((size_t)a.K + wg)] = terms;
        a.stats[2 * ((size_t)a.K + wg) + 1] = substeps;
    }
}

// g_kn = -2 Re <<Xi_k | rho_k(t_n)>> = Re tr(D_k rho_k(t_n)) for every stored state: grid K (N_T + 1), 256 threads, element-wise
// from the store, reduced in a fixed order (the strided partial sums of the threads, then the tree of gb_kernel).  Writes
// gb[K][N_T+1] for jb_reduce_kernel.
struct LindGbArgs {
    const double *Xi;      // [Kd][2][NP*NP] planar
    size_t stride_k;       // doubles: 0 or 2 NP^2
    const double *store;   // [K][N_T+1][2][NP*NP]
    double *gb;            // [K][N_T+1]
    int NP2, N_T;
};
__global__ void __launch_bounds__(256) lind_gb_kernel(LindGbArgs a) {
    __shared__ double part[256];
    const int tid = threadIdx.x, cell = blockIdx.x;   // k * (N_T+1) + n
    const int k = cell / (a.N_T + 1);
    const double *x = a.Xi + (size_t)k * a.stride_k, *r = a.store + (size_t)cell * 2 * a.NP2;
    double acc = 0.;
    for (int i = tid; i < 2 * a.NP2; i += 256) acc += x[i] * r[i];
    part[tid] = acc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    if (tid == 0) a.gb[cell] = -2.0 * part[0];
}
