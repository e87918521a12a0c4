// grape_lindblad_tg.hip.h -- open-system GRAPE: the derivative of J with respect to the time steps (grape_open_time_gradient).
//
// exp(L_n dt_n) commutes with L_n, so on interval n of trajectory k
//     d rho_k(T) / d dt_n = (later steps) L_kn rho_k(t_{n+1})
//     dJ / d dt_n = -2 Re sum_k <<chi_k(t_{n+1}) | L_kn rho_k(t_{n+1})>> = -2 Re sum_k <<L_kn^dagger chi_k(t_{n+1}) | rho_k(t_{n+1})>>
// rho_k(t_{n+1}) is a stored forward state, and L_kn^dagger chi_k(t_{n+1}) is the first term of the adjoint series that steps chi
// back over interval n, before that term is scaled by dt / m.  The kernel therefore walks the chi chain of the backward
// kernel (the c chain alone: no p chain, no control) and takes one more overlap per interval; the result is exact to
// rounding whatever the number of sub-steps.
//
// Layout: that of lind_forward_kernel -- grid K, one workgroup per trajectory, one wave per 16 x 16 tile ((NP / 16)^2 waves),
// the running sum of the chi chain in the registers of the wave that owns the tile, workspace M | M^dagger | C[2] | T[J]
// (the forward kernel's size).  The two partial sums of the overlap travel through the LDS round of the norms: no barrier
// beyond those of the series.  Everything is linear in chi, so chi_k(T) is neither normalised nor rescaled afterwards (the
// stopping rule of a series is relative); the norm guard was the backward half's to report.  Reductions have a fixed order
// (wave butterfly, then the waves by index): results are bitwise repeatable.  No scratch memory.
#pragma once
#include "grape_lindblad.hip.h"

// LindArgs as for lind_backward_kernel, with tg -> [K][N_T] terms <<L^dagger chi_k(t_{n+1}) | rho_k(t_{n+1})>> (out), store an
// input; rho, stats, Dc are not used.  flags[0] |= 16: a series did not converge.
template <int NP>
__global__ void __launch_bounds__(NP * NP / 4) lind_timegrad_kernel(LindArgs a) {
    constexpr int T = NP / 16, NW = T * T, NTH = 64 * NW, NP2 = NP * NP;
    __shared__ double red[2][4][NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, ti = wave / T, tj = wave - ti * T;
    const unsigned aoff = (16 * ti + (lane & 15)) * NP + (lane >> 4), boff = (lane >> 4) * NP + 16 * tj + (lane & 15);
    unsigned o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (16 * ti + 4 * r + (lane >> 4)) * NP + 16 * tj + (lane & 15);
    const int J = a.J, N_T = a.N_T;
    double *ws = a.ws + (size_t)k * (4 + J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *Cb = ws + 4 * NP2, *Tm = ws + 8 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    const double *st = a.store + (size_t)k * (N_T + 1) * 2 * NP2;

    // chi_k(T) = c_k sigma_k of the built-in functionals (include/grape_hip.h) or the caller's
    d4 sr, si;
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
        lind_gd *C0 = lind_uniform(Cb);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double tr = sg[o[r]], tim = sg[NP2 + o[r]];
            sr[r] = cfr * tr - cfi * tim; si[r] = cfr * tim + cfi * tr;
            C0[o[r]] = sr[r]; C0[NP2 + o[r]] = si[r];
        }
    }
    int cur = 0, par = 0, maxo = LIND_MAX_ORDER;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int step = 0; step < N_T; ++step) {
        const int n = N_T - 1 - step;
        const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
        const int msub = lind_substeps(beta, a.dts[n], a.theta);
        const double dt = a.dts[n] / (double)msub;
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            bool conv = false;
            int aord = 0;
            for (; aord < maxo && !conv; ++aord) {
                const double *X = Cb + (size_t)cur * 2 * NP2;
                lind_gd *Y = lind_uniform(Cb + (size_t)(cur ^ 1) * 2 * NP2);
                if (J > 0) {
                    lind_left_products<NP>(Tm, A + 2 * NP2, X, J, aoff, boff, o);
                    __syncthreads();
                }
                d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                lind_apply_tile<NP>(cr, ci, Md, M, X, Tm, A, J, aoff, boff);
                const bool first = sub == 0 && aord == 0;   // (uniform) the unscaled accumulator is L^dagger chi(t_{n+1})
                const double fac = dt * c_series_inv[aord & 255];
                double t2 = 0., s2 = 0., dr = 0., di = 0.;
                const lind_gd *x = lind_uniform(st + (size_t)(n + 1) * 2 * NP2);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (first) {
                        const double xr = x[o[r]], xi = x[NP2 + o[r]];
                        dr += cr[r] * xr + ci[r] * xi;
                        di += cr[r] * xi - ci[r] * xr;
                    }
                    const double ur = fac * cr[r], ui = fac * ci[r];
                    Y[o[r]] = ur; Y[NP2 + o[r]] = ui;
                    sr[r] += ur; si[r] += ui;
                    t2 += ur * ur + ui * ui;
                    s2 += sr[r] * sr[r] + si[r] * si[r];
                }
                if (first) { dr = wave_sum(dr); di = wave_sum(di); }
                t2 = wave_sum(t2); s2 = wave_sum(s2);
                if (lane == 0) {
                    red[par][0][wave] = t2; red[par][1][wave] = s2;
                    if (first) { red[par][2][wave] = dr; red[par][3][wave] = di; }
                }
                __syncthreads();
                t2 = 0.; s2 = 0.;
#pragma unroll
                for (int w = 0; w < NW; ++w) { t2 += red[par][0][w]; s2 += red[par][1][w]; }
                if (first && tid == 0) {
                    dr = 0.; di = 0.;
                    for (int w = 0; w < NW; ++w) { dr += red[par][2][w]; di += red[par][3][w]; }
                    a.tg[(size_t)k * N_T + n] = make_double2(dr, di);
                }
                par ^= 1; cur ^= 1;
                conv = t2 <= tol2 * s2;
            }
            if (!conv) { failed = true; maxo = 1; }
            // chi of the next (sub-)step: C[cur] holds the last term, which nobody reads any more
            lind_gd *X = lind_uniform(Cb + (size_t)cur * 2 * NP2);
#pragma unroll
            for (int r = 0; r < 4; ++r) { X[o[r]] = sr[r]; X[NP2 + o[r]] = si[r]; }
            __syncthreads();
        }
    }
    if (failed && tid == 0) atomicOr(&a.flags[0], 16);
}
