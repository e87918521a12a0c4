// grape_lindblad_batch.hip.h -- many pulse vectors through the problem of one open-system handle (grape_open_eval_batch,
// DESIGN.md 17).
//
// An evaluation on an open-system handle is a latency chain on K (forward) and K L (backward) of the 256 CUs, and its time
// does not depend on K.  Multi-start, a population of optimisers, the trial points of a line search and an
// amplitude scan evaluate the SAME problem at DIFFERENT pulsevals: here the pulse set is one more grid axis, as in
// grape_batch.hip.h for closed handles.  Everything a set owns is reached through pointers of LindArgs (eps, store, ws,
// tau | sums, ||chi||, tau_grads, flags, statistics); a batched kernel rebases those by the strides of one set and runs the
// arithmetic of the ordinary kernel (grape_lindblad.hip.h) on the helpers they share: lind_mac, lind_left_products,
// lind_apply_tile, lind_build_generator, lind_substeps, lind_tile.  The two kernels below repeat the text of lind_forward_kernel /
// lind_backward_kernel after the rebase instead of calling a body moved out of them, as grape_lindblad_hvp.hip.h does: with the
// bodies in __device__ __forceinline__ functions the compiler allocated the registers of the eight ordinary instantiations
// differently (other SGPR spill counts, 75 -> 77 VGPRs at NP = 16), and those kernels are to stay what they were, instruction
// for instruction.  A change to the arithmetic of one file belongs in the other.  Consequences of the layout:
//   - a set computes exactly what the same body computes for it in any other batch or launch group: nothing inside a
//     workgroup depends on gridDim or on the set index, there is no dependency between workgroups, every reduction keeps
//     the fixed order of the ordinary kernels and is segmented over p -- a set does not see its neighbours, bit for bit;
//   - f = sum_k w_k tau_k of set p is read from the sums the reduction of that set left on the device: no host round
//     trip between the forward and the backward launch;
//   - flags are per set, one word for the forward and one for the backward sweep: a series that does not converge or a chi
//     below chi_min_norm is reported for the set and the half that had it;
//   - the static problem (operators, norm estimates, rho_0, targets, weights, shape, dts) is shared, nothing is replicated.
// No floating-point atomics, no scratch memory, 1 KB of LDS, as the ordinary kernels.
#pragma once
#include "grape_lindblad.hip.h"

// element strides from the buffers of one pulse set to those of the next
struct LindBatchStrides {
    size_t eps;     // doubles: L N_T
    size_t store;   // doubles: K (N_T + 1) 2 NP^2
    size_t ws;      // doubles: K L (8 + 2J) 2 NP^2 (the K (4 + J) matrices of the forward workgroups fit inside)
    size_t out;     // doubles: [tau (2K) | sums (8)]
    size_t k;       // K: ||chi_k(T)||
    size_t tg;      // double2: K L N_T
    size_t flags;   // ints: 8 ([0]: the forward launch, [1]: the backward launch -- the host hands the latter flags + 1)
    size_t stats;   // K + K L pairs (series terms, (sub-)steps)
};

__device__ __forceinline__ void lind_batch_rebase(LindArgs &a, const LindBatchStrides &st, const size_t p) {
    a.eps += p * st.eps;
    a.store += p * st.store;
    a.ws += p * st.ws;
    a.tau = (double2 *)((double *)a.tau + p * st.out);
    a.f = (const double *)a.tau + 2 * (size_t)a.K;   // the sums of this set (tau_reduce_body), f = the first two
    a.rho += p * st.k;
    a.tg += p * st.tg;
    a.flags += p * st.flags;
    a.stats += p * st.stats;
}

// grid (K, P): the forward sweep of lind_forward_kernel for trajectory blockIdx.x of set blockIdx.y
template <int NP>
__global__ void __launch_bounds__(NP * NP / 4) lind_batch_forward_kernel(LindArgs a, LindBatchStrides bs) {
    lind_batch_rebase(a, bs, blockIdx.y);
    constexpr int T = NP / 16, NW = T * T, NTH = 64 * NW, NP2 = NP * NP;
    __shared__ double red[2][2][NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, ti = wave / T, tj = wave - ti * T;
    const unsigned aoff = (16 * ti + (lane & 15)) * NP + (lane >> 4), boff = (lane >> 4) * NP + 16 * tj + (lane & 15);
    unsigned o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (16 * ti + 4 * r + (lane >> 4)) * NP + 16 * tj + (lane & 15);
    const int J = a.J, N_T = a.N_T;
    double *ws = a.ws + (size_t)k * (4 + J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *Ub = ws + 4 * NP2, *Tm = ws + 8 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    lind_gd *st = lind_uniform(a.store + (size_t)k * (N_T + 1) * 2 * NP2);

    d4 sr, si;
    {
        const lind_gd *r0 = lind_uniform(a.rho0 + (size_t)k * 2 * NP2);
        lind_gd *U0 = lind_uniform(Ub);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sr[r] = r0[o[r]]; si[r] = r0[NP2 + o[r]];
            st[o[r]] = sr[r]; st[NP2 + o[r]] = si[r];
            U0[o[r]] = sr[r]; U0[NP2 + o[r]] = si[r];
        }
    }
    int cur = 0, par = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int n = 0; n < N_T; ++n) {
        const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
        const int msub = lind_substeps(beta, a.dts[n], a.theta);
        const double dt = a.dts[n] / (double)msub;
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            bool conv = false;
            int aord = 0;
            for (; aord < maxo && !conv; ++aord) {
                const double *X = Ub + (size_t)cur * 2 * NP2;
                lind_gd *Y = lind_uniform(Ub + (size_t)(cur ^ 1) * 2 * NP2);
                if (J > 0) {
                    lind_left_products<NP>(Tm, A, X, J, aoff, boff, o);
                    __syncthreads();
                }
                d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                lind_apply_tile<NP>(cr, ci, M, Md, X, Tm, A + 2 * NP2, J, aoff, boff);
                const double fac = dt * c_series_inv[aord & 255];
                double t2 = 0., s2 = 0.;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double ur = fac * cr[r], ui = fac * ci[r];
                    Y[o[r]] = ur; Y[NP2 + o[r]] = ui;
                    sr[r] += ur; si[r] += ui;
                    t2 += ur * ur + ui * ui;
                    s2 += sr[r] * sr[r] + si[r] * si[r];
                }
                t2 = wave_sum(t2); s2 = wave_sum(s2);
                if (lane == 0) { red[par][0][wave] = t2; red[par][1][wave] = s2; }
                __syncthreads();
                t2 = 0.; s2 = 0.;
#pragma unroll
                for (int w = 0; w < NW; ++w) { t2 += red[par][0][w]; s2 += red[par][1][w]; }
                par ^= 1; cur ^= 1;
                conv = t2 <= tol2 * s2;
            }
            if (!conv) { failed = true; maxo = 1; }
            terms += (unsigned long long)aord;
            ++substeps;
            // the new state is u_0 of the next (sub-)step: U[cur] holds the last term, which nobody reads any more
            lind_gd *X = lind_uniform(Ub + (size_t)cur * 2 * NP2);
#pragma unroll
            for (int r = 0; r < 4; ++r) { X[o[r]] = sr[r]; X[NP2 + o[r]] = si[r]; }
            __syncthreads();
        }
        lind_gd *sn = lind_uniform(st + (size_t)(n + 1) * 2 * NP2);
#pragma unroll
        for (int r = 0; r < 4; ++r) { sn[o[r]] = sr[r]; sn[NP2 + o[r]] = si[r]; }
    }
    {   // tau_k = <<sigma_k | rho_k(T)>> = tr(sigma_k^dagger rho_k(T))
        const lind_gd *tg = lind_uniform(a.target + (size_t)k * 2 * NP2);
        double pr = 0., pi = 0.;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double tr = tg[o[r]], tim = tg[NP2 + o[r]];
            pr += tr * sr[r] + tim * si[r];
            pi += tr * si[r] - tim * sr[r];
        }
        pr = wave_sum(pr); pi = wave_sum(pi);
        if (lane == 0) { red[par][0][wave] = pr; red[par][1][wave] = pi; }
        __syncthreads();
        if (tid == 0) {
            pr = 0.; pi = 0.;
            for (int w = 0; w < NW; ++w) { pr += red[par][0][w]; pi += red[par][1][w]; }
            a.tau[k] = make_double2(pr, pi);
            if (failed) atomicOr(&a.flags[0], 16);
            a.stats[2 * (size_t)k] = terms;
            a.stats[2 * (size_t)k + 1] = substeps;
        }
    }
}

// grid (K, L, P): the backward sweep and gradient of lind_backward_kernel for (trajectory blockIdx.x, control blockIdx.y) of set
// blockIdx.z
template <int NP>
__global__ void __launch_bounds__(LindBwd<NP>::NTH) lind_batch_backward_kernel(LindArgs a, LindBatchStrides bs) {
    lind_batch_rebase(a, bs, blockIdx.z);
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
    int par = 0;

    // chi_k(T) = c_k sigma_k of the built-in functionals (include/grape_hip.h) or the caller's; rho_k = ||chi_k||_F; chi_k /= rho_k
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
        lind_gd *C0 = lind_uniform(Cb);
        double n2 = 0.;
        for (int t = 0; t < TPW; ++t) {
            const LindTile g = lind_tile<NP>(wave * TPW + t, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double tr = sg[g.o[r]], tim = sg[NP2 + g.o[r]];
                const double vr = cfr * tr - cfi * tim, vi = cfr * tim + cfi * tr;
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
        __syncthreads();
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
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        a.stats[2 * ((size_t)a.K + wg)] = terms;
        a.stats[2 * ((size_t)a.K + wg) + 1] = substeps;
    }
}

// the partial sums of every set, each in the order of tau_reduce_kernel; grid (1, P), one wave
__global__ void lind_batch_tau_reduce_kernel(double *out, const double *weights, int K, LindBatchStrides st) {
    double *o = out + (size_t)blockIdx.y * st.out;
    tau_reduce_body((const double2 *)o, weights, K, o + 2 * (size_t)K);
}

// G_p[l N_T + n] = -2 Re sum_k tau_grads[p][k][l][n] in the fixed order of grad_reduce_kernel; grid (ceil(L N_T / 16), P)
__global__ void __launch_bounds__(256) lind_batch_grad_reduce_kernel(double2 *tg, int K, int LN, double *G, LindBatchStrides st) {
    const size_t p = blockIdx.y;
    grad_reduce_body(tg + p * st.tg, K, LN, G + p * (size_t)LN, (const double2 *)nullptr);
}
