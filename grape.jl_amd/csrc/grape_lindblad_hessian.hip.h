// grape_lindblad_hessian.hip.h -- open-system GRAPE: the exact Hessian of J as a matrix on the stored density matrices
// (grape_open_hessian).
//
// grape_open_hvp gives H v; L N_T unit directions give H, but a unit direction e_(m,l') pays two full sweeps and a four-chain
// backward recursion per control for a tangent that is zero before t_m and merely propagated after t_{m+1}.  Written out per
// trajectory in the notation of grape_lindblad_hvp.hip.h, with <<Y|X>> = tr(Y^dagger X), E_n = exp(dt_n L_n): t_n -> t_{n+1}
// and D_nl(X) = s_ln (D_l X + X D_l^dagger), D_l = -i H_l,
//     theta_k(T) = sigma_k,   theta_k(t_n) = E_n^dagger theta_k(t_{n+1})         the BARE target chain (defined when c_k = 0)
//     a_(n,l)    = DE_n[D_nl] rho_k(t_n)                                         lives at t_{n+1}
//     beta_(n,l) = DE_n[D_nl]^dagger theta_k(t_{n+1})                            lives at t_n
//     T_k,p      = d tau_k / d eps_p = <<beta_p | rho_k(t_n)>>                   p = (n, l)
//     S_k,pq     = <<beta_(n,l) | E_{n-1} ... E_{m+1} a_(m,l')>>                 m < n  (empty product for n = m + 1)
//                = <<theta_k(t_{n+1}) | D^2E_n[D_nl, D_nl'] rho_k(t_n)>>         m = n;   symmetric in p <-> q
//     H_pq = -2 Re sum_k [ conj(c_k) S_k,pq + conj(d_q c_k) T_k,p ]              c_k, d_q c_k as in grape_hessian.hip.h
// the formulas of grape_hessian.hip.h with matrices for vectors and the Lindblad series for the propagator.
//
//   lind_hess_forward_seeds_kernel   grid (K, rows, L): block (k, g, l) takes the intervals n = g, g + rows, ... (independent:
//                                    rho_k(t_n) is stored).  The recursion of lind_hvp_forward_kernel for the direction e_(n,l)
//                                    with u'_0 = 0 at every interval:  u_{a+1} = h / (a+1) L u_a,
//                                    a_{a+1} = h / (a+1) (L a_a + D_nl u_a).  Workspace M | M^dagger | U[2] | U'[2] | T[J] | T'[J].
//   lind_hess_theta_kernel           grid (K), sequential in n from the bare sigma_k: the series of lind_forward_kernel under
//                                    L^dagger, one chain.  Stores theta_k(t_n) for every grid point -- which makes the intervals
//                                    of the backward seeds independent, as the stored rho_k(t_n) makes those of the forward
//                                    seeds.  (One workgroup per pair walking all N_T intervals with its four chains was the
//                                    longest serial chain of the call by far: DESIGN.md 26.)  Workspace M | M^dagger | U[2] | T[J].
//   lind_hess_backward_seeds_kernel  grid (K, pairs (l, l' <= l), rows): block (k, pair, g) takes n = N_T - 1 - g, ... with stride
//                                    rows.  The four chains of lind_hvp_backward_kernel with c -> theta, B -> D_nl',
//                                    c' -> beta_l', p -> beta_l, p' -> beta2_ll' (for l = l' the recursion yields the factor 2 of
//                                    D^2E[D, D] by itself); theta starts from the stored theta_k(t_{n+1}), beta_l, beta_l', beta2
//                                    from zero at every interval.  The diagonal pairs store beta_(n,l) and T; every pair stores
//                                    S_diag = <<beta2 | rho_k(t_n)>>.
//                                    Workspace M | M^dagger | C[2] | C'[2] | P[2] | P'[2] | four sums | Tc[4][J].
//   lind_hess_fan_kernel             grid (column blocks, trajectories of the pass).  Columns interval-major, q = m L + l'; a
//                                    workgroup owns `cb` columns and walks n from the birth of its first column: M, M^dagger
//                                    once per n, then column by column -- load it when it is born at t_n, write
//                                    Re(conj(c_k) <<beta_(n,l) | X_q>>) for every l into the strip of the trajectory, carry
//                                    it through interval n (not the last) with the series of lind_forward_kernel.  A column
//                                    is a series of its own: its bits depend neither on its block-mates nor on cb.
//                                    Workspace M | M^dagger | U[2] | T[J] | X[cb].
//   hess_accumulate_kernel, hess_finish_kernel of grape_hessian.hip.h as they are, on a HessArgs filled from the open handle.
// Series as in the Lindblad kernels: m = ceil(beta_n dt_n / theta) sub-steps with the handle's beta_n and all chains carried
// over, a series stops when EVERY chain has ||term||_F <= tol ||sum||_F (an identically zero chain counts as converged), after
// at most LIND_MAX_ORDER terms (flag 16 otherwise).  MFMA operands come from the L2-resident workspace, base addresses pinned
// with lind_uniform.  Reductions in a fixed order (wave butterfly, then the waves by index).  No floating-point atomics, no
// scratch memory.
#pragma once
#include "grape_lindblad_hvp.hip.h"
#include "grape_hessian.hip.h"

struct LindHessArgs {
    LindArgs a;             // the problem, eps, tau, f, store (stored rho_k(t_n): an input); flags: the word of this call
    double *av;             // [K][N_T][L][2][NP*NP] a_(n,l)
    double *bv;             // [K][N_T][L][2][NP*NP] beta_(n,l)
    double *th;             // [K][N_T+1][2][NP*NP] theta_k(t_n)
    double2 *T;             // [K][N_T*L] T_k,(n,l)
    double2 *Sd;            // [K][N_T][HESS_PAIRS] S_k,(n,l)(n,l'), pair l (l + 1) / 2 + l', l' <= l
    double *strip;          // [trajectories of the pass][P][P] rows (n, l), columns (m, l'); written for m < n only
    double *ws;             // workspaces of the launch
    unsigned long long *stats;   // [workgroups][2] series terms, (sub-)steps of the launch
    int k0;                 // first trajectory of the pass
    int cb;                 // columns per workgroup of the fan
};

// ---------------------------------------------------------------------------------------
// Forward seeds a_(n,l) = DE_n[D_nl] rho_k(t_n): grid (K, rows, L); block (k, g, l) takes n = g, g + rows, ...
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(NP * NP / 4) lind_hess_forward_seeds_kernel(LindHessArgs q) {
    constexpr int T = NP / 16, NW = T * T, NTH = 64 * NW, NP2 = NP * NP;
    __shared__ double red[2][4][NW];
    const LindArgs &a = q.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, l = blockIdx.z;   // (the wave's tile is tile `wave`: lind_hvp_tile where a section needs the offsets)
    const int J = a.J, N_T = a.N_T, L = a.L;
    const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + k;
    double *ws = q.ws + wg * (6 + 2 * J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *Ub = ws + 4 * NP2, *Vb = ws + 8 * NP2;
    double *Tm = ws + 12 * NP2, *Tv = Tm + (size_t)J * 2 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    const double *Dl = a.Dc + ((size_t)(a.hc_per_traj ? k : 0) * L + l) * 4 * NP2, *Dld = Dl + 2 * NP2;
    const double *st = a.store + (size_t)k * (N_T + 1) * 2 * NP2;

    int cur = 0, par = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int n = blockIdx.y; n < N_T; n += gridDim.y) {
        const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
        const int msub = lind_substeps(beta, a.dts[n], a.theta);
        const double dt = a.dts[n] / (double)msub;
        const double sh = a.shape ? a.shape[(size_t)l * N_T + n] : 1.0;
        d4 sr, si, pr = (d4){0., 0., 0., 0.}, pi = (d4){0., 0., 0., 0.};
        {   // u_0 = the stored rho_k(t_n), u'_0 = 0
            const LindTile g = lind_hvp_tile<NP>(wave, lane);
            const lind_gd *x = lind_uniform(st + (size_t)n * 2 * NP2);
            lind_gd *U0 = lind_uniform(Ub + (size_t)cur * 2 * NP2), *V0 = lind_uniform(Vb + (size_t)cur * 2 * NP2);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sr[r] = x[g.o[r]]; si[r] = x[NP2 + g.o[r]];
                U0[g.o[r]] = sr[r]; U0[NP2 + g.o[r]] = si[r];
                V0[g.o[r]] = 0.; V0[NP2 + g.o[r]] = 0.;
            }
        }
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            bool conv = false;
            int aord = 0;
            for (; aord < maxo && !conv; ++aord) {
                const LindTile g = lind_hvp_tile<NP>(wave, lane);
                const double *X = Ub + (size_t)cur * 2 * NP2, *Xp = Vb + (size_t)cur * 2 * NP2;
                lind_gd *Y = lind_uniform(Ub + (size_t)(cur ^ 1) * 2 * NP2), *Yp = lind_uniform(Vb + (size_t)(cur ^ 1) * 2 * NP2);
                if (J > 0) {
                    lind_left_products<NP>(Tm, A, X, J, g.aoff, g.boff, g.o);
                    lind_left_products<NP>(Tv, A, Xp, J, g.aoff, g.boff, g.o);
                    __syncthreads();
                }
                const double fac = dt * c_series_inv[aord & 255];
                double t2 = 0., s2 = 0., tp2 = 0., sp2 = 0.;
                {
                    d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                    lind_apply_tile<NP>(cr, ci, M, Md, X, Tm, A + 2 * NP2, J, g.aoff, g.boff);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ur = fac * cr[r], ui = fac * ci[r];
                        Y[g.o[r]] = ur; Y[NP2 + g.o[r]] = ui;
                        sr[r] += ur; si[r] += ui;
                        t2 += ur * ur + ui * ui;
                        s2 += sr[r] * sr[r] + si[r] * si[r];
                    }
                }
                {   // D_nl u = s_ln (D_l u + u D_l^dagger), then L a
                    d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                    lind_mac<NP>(cr, ci, Dl, X, g.aoff, g.boff);
                    lind_mac<NP>(cr, ci, X, Dld, g.aoff, g.boff);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { cr[r] *= sh; ci[r] *= sh; }
                    lind_apply_tile<NP>(cr, ci, M, Md, Xp, Tv, A + 2 * NP2, J, g.aoff, g.boff);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ur = fac * cr[r], ui = fac * ci[r];
                        Yp[g.o[r]] = ur; Yp[NP2 + g.o[r]] = ui;
                        pr[r] += ur; pi[r] += ui;
                        tp2 += ur * ur + ui * ui;
                        sp2 += pr[r] * pr[r] + pi[r] * pi[r];
                    }
                }
                t2 = wave_sum(t2); s2 = wave_sum(s2); tp2 = wave_sum(tp2); sp2 = wave_sum(sp2);
                if (lane == 0) { red[par][0][wave] = t2; red[par][1][wave] = s2; red[par][2][wave] = tp2; red[par][3][wave] = sp2; }
                __syncthreads();
                t2 = 0.; s2 = 0.; tp2 = 0.; sp2 = 0.;
#pragma unroll
                for (int w = 0; w < NW; ++w) { t2 += red[par][0][w]; s2 += red[par][1][w]; tp2 += red[par][2][w]; sp2 += red[par][3][w]; }
                par ^= 1; cur ^= 1;
                conv = t2 <= tol2 * s2 && tp2 <= tol2 * sp2;
            }
            if (!conv) { failed = true; maxo = 1; }
            terms += (unsigned long long)aord;
            ++substeps;
            // (u, a) of the next sub-step: the buffers of the last terms are no longer read by anyone
            lind_gd *X = lind_uniform(Ub + (size_t)cur * 2 * NP2), *Xp = lind_uniform(Vb + (size_t)cur * 2 * NP2);
            const LindTile g = lind_hvp_tile<NP>(wave, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) { X[g.o[r]] = sr[r]; X[NP2 + g.o[r]] = si[r]; Xp[g.o[r]] = pr[r]; Xp[NP2 + g.o[r]] = pi[r]; }
            __syncthreads();
        }
        lind_gd *out = lind_uniform(q.av + (((size_t)k * N_T + n) * L + l) * 2 * NP2);
        const LindTile g = lind_hvp_tile<NP>(wave, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) { out[g.o[r]] = pr[r]; out[NP2 + g.o[r]] = pi[r]; }
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        q.stats[2 * wg] = terms;
        q.stats[2 * wg + 1] = substeps;
    }
}

// ---------------------------------------------------------------------------------------
// The bare target chain theta_k(t_n) = E_n^dagger theta_k(t_{n+1}) from theta_k(T) = sigma_k: grid (K), sequential in n.
// lind_forward_kernel with L^dagger for L (one chain, 2 + 2J products per term).  Workspace M | M^dagger | U[2] | T[J].
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(NP * NP / 4) lind_hess_theta_kernel(LindHessArgs q) {
    constexpr int T = NP / 16, NW = T * T, NTH = 64 * NW, NP2 = NP * NP;
    __shared__ double red[2][2][NW];
    const LindArgs &a = q.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, ti = wave / T, tj = wave - ti * T;
    const unsigned aoff = (16 * ti + (lane & 15)) * NP + (lane >> 4), boff = (lane >> 4) * NP + 16 * tj + (lane & 15);
    unsigned o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (16 * ti + 4 * r + (lane >> 4)) * NP + 16 * tj + (lane & 15);
    const int J = a.J, N_T = a.N_T;
    double *ws = q.ws + (size_t)k * (4 + J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *Ub = ws + 4 * NP2, *Tm = ws + 8 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    lind_gd *th = lind_uniform(q.th + (size_t)k * (N_T + 1) * 2 * NP2);

    d4 sr, si;
    {
        const lind_gd *sg = lind_uniform(a.target + (size_t)k * 2 * NP2);
        lind_gd *U0 = lind_uniform(Ub), *tT = lind_uniform(th + (size_t)N_T * 2 * NP2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sr[r] = sg[o[r]]; si[r] = sg[NP2 + o[r]];
            tT[o[r]] = sr[r]; tT[NP2 + o[r]] = si[r];
            U0[o[r]] = sr[r]; U0[NP2 + o[r]] = si[r];
        }
    }
    int cur = 0, par = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int n = N_T - 1; n >= 0; --n) {
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
                    lind_left_products<NP>(Tm, A + 2 * NP2, X, J, aoff, boff, o);
                    __syncthreads();
                }
                d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                lind_apply_tile<NP>(cr, ci, Md, M, X, Tm, A, J, aoff, boff);
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
            // the new theta is u_0 of the next (sub-)step: U[cur] holds the last term, which nobody reads any more
            lind_gd *X = lind_uniform(Ub + (size_t)cur * 2 * NP2);
#pragma unroll
            for (int r = 0; r < 4; ++r) { X[o[r]] = sr[r]; X[NP2 + o[r]] = si[r]; }
            __syncthreads();
        }
        lind_gd *tn = lind_uniform(th + (size_t)n * 2 * NP2);
#pragma unroll
        for (int r = 0; r < 4; ++r) { tn[o[r]] = sr[r]; tn[NP2 + o[r]] = si[r]; }
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        q.stats[2 * (size_t)k] = terms;
        q.stats[2 * (size_t)k + 1] = substeps;
    }
}

// ---------------------------------------------------------------------------------------
// Backward seeds: grid (K, pairs, rows), pair = l (l + 1) / 2 + l', l' <= l; block (k, pair, g) takes the intervals
// n = N_T - 1 - g, N_T - 1 - g - rows, ... (independent: theta_k(t_{n+1}) is stored).
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(LindBwd<NP>::NTH) lind_hess_backward_seeds_kernel(LindHessArgs q) {
    constexpr int TPW = LindBwd<NP>::TPW, NW = LindBwd<NP>::NW, NTH = LindBwd<NP>::NTH, NP2 = NP * NP;
    __shared__ double red[2][8][NW];
    const LindArgs &a = q.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, pair = blockIdx.y;
    int l = 0;
    while ((l + 1) * (l + 2) / 2 <= pair) ++l;
    const int l2 = pair - l * (l + 1) / 2;
    const int J = a.J, N_T = a.N_T, L = a.L;
    const size_t wg = ((size_t)blockIdx.z * gridDim.y + pair) * a.K + k;
    double *ws = q.ws + wg * (14 + 4 * J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2;
    double *Cb = ws + 4 * NP2, *Cpb = ws + 8 * NP2, *Pb = ws + 12 * NP2, *Ppb = ws + 16 * NP2;
    lind_gd *Cs = lind_uniform(ws + 20 * NP2), *Cps = lind_uniform(ws + 22 * NP2), *Ps = lind_uniform(ws + 24 * NP2),
            *Pps = lind_uniform(ws + 26 * NP2);
    double *Tc = ws + 28 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    const double *Dl = a.Dc + ((size_t)(a.hc_per_traj ? k : 0) * L + l) * 4 * NP2, *Dld = Dl + 2 * NP2;
    const double *Dv = a.Dc + ((size_t)(a.hc_per_traj ? k : 0) * L + l2) * 4 * NP2, *Dvd = Dv + 2 * NP2;
    const double *st = a.store + (size_t)k * (N_T + 1) * 2 * NP2;
    int par = 0;

    int cur = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int n = N_T - 1 - (int)blockIdx.z; n >= 0; n -= (int)gridDim.z) {
        const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
        const int msub = lind_substeps(beta, a.dts[n], a.theta);
        const double dt = a.dts[n] / (double)msub;
        const double sh = a.shape ? a.shape[(size_t)l * N_T + n] : 1.0, shv = a.shape ? a.shape[(size_t)l2 * N_T + n] : 1.0;
        {   // theta starts from the stored theta_k(t_{n+1}); beta_l' = beta_l = beta2 = 0 at the start of every interval
            const lind_gd *tq = lind_uniform((const double *)q.th + ((size_t)k * (N_T + 1) + n + 1) * 2 * NP2);
            lind_gd *C0 = lind_uniform(Cb + (size_t)cur * 2 * NP2);
            lind_gd *Cp0 = lind_uniform(Cpb + (size_t)cur * 2 * NP2), *P0 = lind_uniform(Pb + (size_t)cur * 2 * NP2),
                    *Pp0 = lind_uniform(Ppb + (size_t)cur * 2 * NP2);
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double tr = tq[g.o[r]], tim = tq[NP2 + g.o[r]];
                    Cs[g.o[r]] = tr; Cs[NP2 + g.o[r]] = tim; C0[g.o[r]] = tr; C0[NP2 + g.o[r]] = tim;
                    Cp0[g.o[r]] = 0.; Cp0[NP2 + g.o[r]] = 0.; Cps[g.o[r]] = 0.; Cps[NP2 + g.o[r]] = 0.;
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
                // the four chains have one layout (term buffers C | C' | P | P', sums, T in that order): chain ch is a run-time
                // index, so that one chain's operands are live at a time (all four side by side spill at NP = 48, 64)
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
                    // theta: L^+ theta | beta_l': D_nl'^+ theta + L^+ beta_l' | beta_l: D_nl^+ theta + L^+ beta_l
                    // beta2: D_nl^+ beta_l' + D_nl'^+ beta_l + L^+ beta2
                    const double *Xd = Xb + (size_t)(ch == 2 ? 0 : 1) * 4 * NP2;   // what D_nl^dagger acts on (ch >= 2)
                    const double *Xv = Xb + (size_t)(ch == 1 ? 0 : 2) * 4 * NP2;   // what D_nl'^dagger acts on (ch odd)
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
                            d4 vr = (d4){0., 0., 0., 0.}, vi = (d4){0., 0., 0., 0.};
                            lind_mac<NP>(vr, vi, Dvd, Xv, g.aoff, g.boff);
                            lind_mac<NP>(vr, vi, Xv, Dv, g.aoff, g.boff);
#pragma unroll
                            for (int r = 0; r < 4; ++r) { cr[r] = fma(shv, vr[r], cr[r]); ci[r] = fma(shv, vi[r], ci[r]); }
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
        {   // T = <<beta_l | rho_k(t_n)>>, S_diag = <<beta2 | rho_k(t_n)>>; the diagonal pair keeps beta_(n,l)
            const lind_gd *x = lind_uniform(st + (size_t)n * 2 * NP2);
            lind_gd *bo = lind_uniform(q.bv + (((size_t)k * N_T + n) * L + l) * 2 * NP2);
            double dr = 0., di = 0., er = 0., ei = 0.;
            for (int t = 0; t < TPW; ++t) {
                const LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double xr = x[g.o[r]], xi = x[NP2 + g.o[r]], ppr = Pps[g.o[r]], ppi = Pps[NP2 + g.o[r]];
                    const double pr = Ps[g.o[r]], pi = Ps[NP2 + g.o[r]];
                    dr += ppr * xr + ppi * xi;
                    di += ppr * xi - ppi * xr;
                    er += pr * xr + pi * xi;
                    ei += pr * xi - pi * xr;
                    if (l == l2) { bo[g.o[r]] = pr; bo[NP2 + g.o[r]] = pi; }
                }
            }
            dr = wave_sum(dr); di = wave_sum(di); er = wave_sum(er); ei = wave_sum(ei);
            if (lane == 0) { red[par][0][wave] = dr; red[par][1][wave] = di; red[par][2][wave] = er; red[par][3][wave] = ei; }
            __syncthreads();
            if (tid == 0) {
                dr = 0.; di = 0.; er = 0.; ei = 0.;
                for (int w = 0; w < NW; ++w) { dr += red[par][0][w]; di += red[par][1][w]; er += red[par][2][w]; ei += red[par][3][w]; }
                q.Sd[((size_t)k * N_T + n) * HESS_PAIRS + pair] = make_double2(dr, di);
                if (l == l2) q.T[(size_t)k * N_T * L + (size_t)n * L + l] = make_double2(er, ei);
            }
            par ^= 1;
        }
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        q.stats[2 * wg] = terms;
        q.stats[2 * wg + 1] = substeps;
    }
}

// ---------------------------------------------------------------------------------------
// Fan: grid (ceil(P / cb), trajectories of the pass).  Block b carries the columns q = cb b .. cb b + cb - 1 (q = m L + l',
// born at t_{m+1}) from the birth of its first column to the last grid point, one column after the other at every n.
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(NP * NP / 4) lind_hess_fan_kernel(LindHessArgs q) {
    constexpr int T = NP / 16, NW = T * T, NTH = 64 * NW, NP2 = NP * NP;
    __shared__ double red[2][2][NW];
    const LindArgs &a = q.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, kk = blockIdx.y, k = q.k0 + kk, ti = wave / T, tj = wave - ti * T;
    const unsigned aoff = (16 * ti + (lane & 15)) * NP + (lane >> 4), boff = (lane >> 4) * NP + 16 * tj + (lane & 15);
    unsigned o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (16 * ti + 4 * r + (lane >> 4)) * NP + 16 * tj + (lane & 15);
    const int J = a.J, N_T = a.N_T, L = a.L, P = L * N_T, cb = q.cb;
    const size_t wg = (size_t)kk * gridDim.x + b;
    double *ws = q.ws + wg * (size_t)(4 + J + cb) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *Ub = ws + 4 * NP2, *Tm = ws + 8 * NP2, *Xc = Tm + (size_t)J * 2 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    double *strip = q.strip + (size_t)kk * P * P;
    double ckr, cki;   // c_k of chi_k(T) = c_k sigma_k at the last evaluation (hess_coef)
    {
        const double w = a.weights ? a.weights[k] : 1.0, Kt = (double)a.K_total;
        if (a.functional == 0) { ckr = w * a.f[0] / (Kt * Kt); cki = w * a.f[1] / (Kt * Kt); }
        else if (a.functional == 1) { const double2 t = a.tau[k]; ckr = w * t.x / Kt; cki = w * t.y / Kt; }
        else { ckr = w / (2.0 * Kt); cki = 0.; }
    }
    int cur = 0, par = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int n = (cb * b) / L + 1; n < N_T; ++n) {
        const bool carry = n < N_T - 1;
        int msub = 1;
        double dt = 0.;
        if (carry) {
            const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
            msub = lind_substeps(beta, a.dts[n], a.theta);
            dt = a.dts[n] / (double)msub;
        }
        __syncthreads();
        for (int c = 0; c < cb; ++c) {
            const int col = cb * b + c, mq = col / L, lq = col - mq * L;   // born at t_{mq + 1}
            if (col >= P || mq >= n) break;                               // (the later columns are younger still)
            d4 sr, si;
            {   // the column at t_n: born now, or as the last interval left it
                const lind_gd *src = mq == n - 1 ? lind_uniform((const double *)q.av + (((size_t)k * N_T + mq) * L + lq) * 2 * NP2)
                                                 : lind_uniform((const double *)Xc + (size_t)c * 2 * NP2);
#pragma unroll
                for (int r = 0; r < 4; ++r) { sr[r] = src[o[r]]; si[r] = src[NP2 + o[r]]; }
            }
            // Re(conj(c_k) <<beta_(n,l) | X_q>>) for every l: the lane's elements, wave butterfly, then the waves by index
            for (int l = 0; l < L; ++l) {
                const lind_gd *bt = lind_uniform((const double *)q.bv + (((size_t)k * N_T + n) * L + l) * 2 * NP2);
                double dr = 0., di = 0.;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double yr = bt[o[r]], yi = bt[NP2 + o[r]];
                    dr += yr * sr[r] + yi * si[r];
                    di += yr * si[r] - yi * sr[r];
                }
                dr = wave_sum(dr); di = wave_sum(di);
                if (lane == 0) { red[par][0][wave] = dr; red[par][1][wave] = di; }
                __syncthreads();
                if (tid == 0) {
                    dr = 0.; di = 0.;
                    for (int w = 0; w < NW; ++w) { dr += red[par][0][w]; di += red[par][1][w]; }
                    strip[((size_t)n * L + l) * P + col] = ckr * dr + cki * di;
                }
                par ^= 1;
            }
            if (!carry) continue;
            {
                lind_gd *U0 = lind_uniform(Ub + (size_t)cur * 2 * NP2);
#pragma unroll
                for (int r = 0; r < 4; ++r) { U0[o[r]] = sr[r]; U0[NP2 + o[r]] = si[r]; }
            }
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
                // the new column is u_0 of the next (sub-)step: U[cur] holds the last term, which nobody reads any more
                lind_gd *X = lind_uniform(Ub + (size_t)cur * 2 * NP2);
#pragma unroll
                for (int r = 0; r < 4; ++r) { X[o[r]] = sr[r]; X[NP2 + o[r]] = si[r]; }
                __syncthreads();
            }
            lind_gd *keep = lind_uniform(Xc + (size_t)c * 2 * NP2);
#pragma unroll
            for (int r = 0; r < 4; ++r) { keep[o[r]] = sr[r]; keep[NP2 + o[r]] = si[r]; }
        }
    }
    if (tid == 0) {
        if (failed) atomicOr(&a.flags[0], 16);
        q.stats[2 * wg] = terms;
        q.stats[2 * wg + 1] = substeps;
    }
}
