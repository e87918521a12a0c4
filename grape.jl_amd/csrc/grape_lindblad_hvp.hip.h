// grape_lindblad_hvp.hip.h -- open-system GRAPE: exact Hessian-vector products of J on the stored density matrices
// (grape_open_hvp).
//
// Notation of grape_lindblad.hip.h.  For a direction v the generator of interval n has the directional derivative
//     B = sum_l v_nl s_ln D_l,      B(X) = B X + X B^dagger,      B^dagger(Y) = B^dagger Y + Y B
// (one more matrix and its adjoint next to M, M^dagger), and the block recursion of DESIGN.md 14 carries over:
//   tangent forward sweep (lind_hvp_forward_kernel), chains u, u' under L:
//       u_0 = rho_k(t_n) (the STORED state),  u'_0 = rho'_k(t_n),  rho'_k(t_0) = 0
//       u_{a+1} = h / (a+1) L u_a,            u'_{a+1} = h / (a+1) (L u'_a + B u_a)
//     rho'_k(t_{n+1}) = sum_a u'_a is stored per direction; tau'_k = <<sigma_k | rho'_k(T)>>.
//   boundary (lind_hvp_boundary_kernel): f' = sum_k w_k tau'_k,  chi'_k(T) = c'_k sigma_k  (sm: w_k f' / K^2, ss: w_k tau'_k / K, re: 0)
//   backward sweep (lind_hvp_backward_kernel), chains c, c', p, p' under L^dagger for ONE control l:
//       c_{a+1}  = h / (a+1) L^dagger c_a                      c'_{a+1} = h / (a+1) (L^dagger c'_a + B^dagger c_a)
//       p_{a+1}  = h / (a+1) (L^dagger p_a + D_l^dagger c_a)   p'_{a+1} = h / (a+1) (L^dagger p'_a + B^dagger p_a + D_l^dagger c'_a)
//     with D_l^dagger (Y) = s_ln (D_l^dagger Y + Y D_l), from c_0 = chi_{n+1}, c'_0 = chi'_{n+1}, p_0 = p'_0 = 0.  The sums are
//     chi_n, chi'_n, P_l, P'_l, and the per-trajectory term of (H v)_nl is <<P'_l | rho_k(t_n)>> + <<P_l | rho'_k(t_n)>>.
//   chi_k(T) = c_k sigma_k with the c_k of the backward kernel's prologue, NOT normalised: everything is linear in chi and the
//   stopping rule is relative.  A long step is cut into m = ceil(beta_n dt_n / theta) sub-steps with the beta_n of the
//   gradient (B does not enter it); all chains carry over from one sub-step to the next.  A series stops when EVERY chain
//   has ||term||_F <= tol ||sum||_F (a chain that is identically zero counts as converged), after at most LIND_MAX_ORDER terms.
//
// Layout on the chip.  Forward: grid (K, directions), the shape of lind_forward_kernel -- one wave per 16 x 16 tile, the
// running sums of u and u' in the registers of the wave that owns the tile, workspace per workgroup
//     M | M^dagger | B | B^dagger | U[2] | U'[2] | T[J] | T'[J]                              (6 + 4J products per term).
// Backward: grid (K, L, directions), waves as LindBwd<NP> (two tiles per wave at NP = 64), the running sums of the four
// chains in the workspace (every lane updates its own elements), workspace per workgroup
//     M | M^dagger | B | B^dagger | C[2] | C'[2] | P[2] | P'[2] | sum C | sum C' | sum P | sum P' | Tc[J] | Tc'[J] | Tp[J] | Tp'[J]
//                                                                                            (16 + 8J products per term).
// MFMA operands come straight from the L2-resident workspace (planar row-major, base addresses pinned with lind_uniform).
// Reductions have a fixed order (wave butterfly, then the waves by index, through the LDS): results are bitwise repeatable,
// and a direction never sees its neighbours -- its result does not depend on nv or on the launch groups.  No floating-point
// atomics, no scratch memory.
#pragma once
#include "grape_lindblad.hip.h"

struct LindHvpArgs {
    LindArgs a;             // the problem, eps, tau, f, store (stored rho_k(t_n): an input), flags of the handle; ws, tg, stats, rho unused
    const double *V;        // [nd][L*N_T] directions of this launch group
    double *dstore;         // [nd][K][N_T+1][2][NP*NP] rho'_k(t_n)
    double2 *dtau;          // [nd][K] tau'_k
    double2 *dcoef;         // [nd][K] c'_k
    double2 *tg;            // [nd][K][L*N_T] per-trajectory terms of H v (input of grad_reduce_kernel)
    double *ws;             // workspaces: nd K (8 + 2J) matrices forward, nd K L (16 + 4J) backward (the same buffer)
    unsigned long long *stats;   // [nd*K][2] forward workgroups, then [nd*K*L][2] backward workgroups: series terms, (sub-)steps
    int nd;
};

// B = sum_l v_nl s_ln D_l and B^dagger of interval n (D_l, D_l^dagger as LindArgs::Dc keeps them)
template <int NP, int NTH>
__device__ __forceinline__ void lind_hvp_build_direction(const LindArgs &a, const double *v, const int k, const int n, double *B, double *Bd) {
    constexpr int NP2 = NP * NP;
    const int L = a.L, N_T = a.N_T;
    const double *Dc = a.Dc + (size_t)(a.hc_per_traj ? k : 0) * L * 4 * NP2;
    lind_gd *Bg = lind_uniform(B), *Bdg = lind_uniform(Bd);
    static_assert(NP2 % NTH == 0, "every thread owns NP2 / NTH elements");
#pragma unroll 1
    for (unsigned it = 0; it < (unsigned)(NP2 / NTH); ++it) {   // (a uniform trip count: no divergent loop next to the pinned bases)
        const unsigned idx = it * NTH + threadIdx.x;
        double br = 0., bi = 0., dr = 0., di = 0.;
        for (int l = 0; l < L; ++l) {
            const double c = v[(size_t)l * N_T + n] * (a.shape ? a.shape[(size_t)l * N_T + n] : 1.0);
            const lind_gd *d = lind_uniform(Dc + (size_t)l * 4 * NP2);
            br = fma(c, d[idx], br);
            bi = fma(c, d[NP2 + idx], bi);
            dr = fma(c, d[2 * NP2 + idx], dr);
            di = fma(c, d[3 * NP2 + idx], di);
        }
        Bg[idx] = br; Bg[NP2 + idx] = bi;
        Bdg[idx] = dr; Bdg[NP2 + idx] = di;
    }
}

// ---------------------------------------------------------------------------------------
// Tangent forward sweep: grid (K, directions), one workgroup per (trajectory, direction).
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(NP * NP / 4) lind_hvp_forward_kernel(LindHvpArgs q) {
    constexpr int T = NP / 16, NW = T * T, NTH = 64 * NW, NP2 = NP * NP;
    __shared__ double red[2][4][NW];
    const LindArgs &a = q.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x, jd = blockIdx.y, ti = wave / T, tj = wave - ti * T;
    const unsigned aoff = (16 * ti + (lane & 15)) * NP + (lane >> 4), boff = (lane >> 4) * NP + 16 * tj + (lane & 15);
    unsigned o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (16 * ti + 4 * r + (lane >> 4)) * NP + 16 * tj + (lane & 15);
    const int J = a.J, N_T = a.N_T;
    const size_t wg = (size_t)jd * a.K + k;
    double *ws = q.ws + wg * (8 + 2 * J) * 2 * NP2;
    double *M = ws, *Md = ws + 2 * NP2, *B = ws + 4 * NP2, *Bd = ws + 6 * NP2, *Ub = ws + 8 * NP2, *Vb = ws + 12 * NP2;
    double *Tm = ws + 16 * NP2, *Tv = Tm + (size_t)J * 2 * NP2;
    const double *A = a.A + (size_t)(a.cops_per_traj ? k : 0) * J * 4 * NP2;
    const double *v = q.V + (size_t)jd * a.L * N_T;
    const double *st = a.store + (size_t)k * (N_T + 1) * 2 * NP2;
    lind_gd *ds = lind_uniform(q.dstore + wg * (size_t)(N_T + 1) * 2 * NP2);

    d4 sr, si, pr = (d4){0., 0., 0., 0.}, pi = (d4){0., 0., 0., 0.};
    {   // rho'_k(t_0) = 0
        lind_gd *V0 = lind_uniform(Vb);
#pragma unroll
        for (int r = 0; r < 4; ++r) { ds[o[r]] = 0.; ds[NP2 + o[r]] = 0.; V0[o[r]] = 0.; V0[NP2 + o[r]] = 0.; }
    }
    int cur = 0, par = 0, maxo = LIND_MAX_ORDER;
    unsigned long long terms = 0, substeps = 0;
    bool failed = false;
    const double tol2 = a.tol * a.tol;

    for (int n = 0; n < N_T; ++n) {
        const double beta = lind_build_generator<NP, NTH>(a, k, n, M, Md);
        lind_hvp_build_direction<NP, NTH>(a, v, k, n, B, Bd);
        const int msub = lind_substeps(beta, a.dts[n], a.theta);
        const double dt = a.dts[n] / (double)msub;
        {   // u_0 = the stored rho_k(t_n)   (U'[cur] holds rho'_k(t_n) already)
            const lind_gd *x = lind_uniform(st + (size_t)n * 2 * NP2);
            lind_gd *U0 = lind_uniform(Ub + (size_t)cur * 2 * NP2);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sr[r] = x[o[r]]; si[r] = x[NP2 + o[r]];
                U0[o[r]] = sr[r]; U0[NP2 + o[r]] = si[r];
            }
        }
        __syncthreads();
        for (int sub = 0; sub < msub; ++sub) {
            bool conv = false;
            int aord = 0;
            for (; aord < maxo && !conv; ++aord) {
                const double *X = Ub + (size_t)cur * 2 * NP2, *Xp = Vb + (size_t)cur * 2 * NP2;
                lind_gd *Y = lind_uniform(Ub + (size_t)(cur ^ 1) * 2 * NP2), *Yp = lind_uniform(Vb + (size_t)(cur ^ 1) * 2 * NP2);
                if (J > 0) {
                    lind_left_products<NP>(Tm, A, X, J, aoff, boff, o);
                    lind_left_products<NP>(Tv, A, Xp, J, aoff, boff, o);
                    __syncthreads();
                }
                const double fac = dt * c_series_inv[aord & 255];
                double t2 = 0., s2 = 0., tp2 = 0., sp2 = 0.;
                {
                    d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                    lind_apply_tile<NP>(cr, ci, M, Md, X, Tm, A + 2 * NP2, J, aoff, boff);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ur = fac * cr[r], ui = fac * ci[r];
                        Y[o[r]] = ur; Y[NP2 + o[r]] = ui;
                        sr[r] += ur; si[r] += ui;
                        t2 += ur * ur + ui * ui;
                        s2 += sr[r] * sr[r] + si[r] * si[r];
                    }
                }
                {
                    d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
                    lind_mac<NP>(cr, ci, B, X, aoff, boff);
                    lind_mac<NP>(cr, ci, X, Bd, aoff, boff);
                    lind_apply_tile<NP>(cr, ci, M, Md, Xp, Tv, A + 2 * NP2, J, aoff, boff);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double ur = fac * cr[r], ui = fac * ci[r];
                        Yp[o[r]] = ur; Yp[NP2 + o[r]] = ui;
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
            // (u, u') of the next (sub-)step: the buffers of the last terms are no longer read by anyone
            lind_gd *X = lind_uniform(Ub + (size_t)cur * 2 * NP2), *Xp = lind_uniform(Vb + (size_t)cur * 2 * NP2);
#pragma unroll
            for (int r = 0; r < 4; ++r) { X[o[r]] = sr[r]; X[NP2 + o[r]] = si[r]; Xp[o[r]] = pr[r]; Xp[NP2 + o[r]] = pi[r]; }
            __syncthreads();
        }
        lind_gd *sn = lind_uniform(ds + (size_t)(n + 1) * 2 * NP2);
#pragma unroll
        for (int r = 0; r < 4; ++r) { sn[o[r]] = pr[r]; sn[NP2 + o[r]] = pi[r]; }
    }
    {   // tau'_k = <<sigma_k | rho'_k(T)>>
        const lind_gd *tg = lind_uniform(a.target + (size_t)k * 2 * NP2);
        double xr = 0., xi = 0.;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double tr = tg[o[r]], tim = tg[NP2 + o[r]];
            xr += tr * pr[r] + tim * pi[r];
            xi += tr * pi[r] - tim * pr[r];
        }
        xr = wave_sum(xr); xi = wave_sum(xi);
        if (lane == 0) { red[par][0][wave] = xr; red[par][1][wave] = xi; }
        __syncthreads();
        if (tid == 0) {
            xr = 0.; xi = 0.;
            for (int w = 0; w < NW; ++w) { xr += red[par][0][w]; xi += red[par][1][w]; }
            q.dtau[wg] = make_double2(xr, xi);
            if (failed) atomicOr(&a.flags[0], 16);
            q.stats[2 * wg] = terms;
            q.stats[2 * wg + 1] = substeps;
        }
    }
}

// f' = sum_k w_k tau'_k and the c'_k of chi'_k(T) = c'_k sigma_k; one wave per direction, fixed order
__global__ void __launch_bounds__(64) lind_hvp_boundary_kernel(LindHvpArgs q) {
    const int jd = blockIdx.x, lane = threadIdx.x, K = q.a.K;
    const double2 *dt = q.dtau + (size_t)jd * K;
    double fr = 0., fi = 0.;
    for (int k = lane; k < K; k += 64) {
        const double w = q.a.weights ? q.a.weights[k] : 1.0;
        fr += w * dt[k].x; fi += w * dt[k].y;
    }
    fr = wave_sum(fr); fi = wave_sum(fi);
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
// Backward sweep: grid (K, L, directions), one control per workgroup.
// ---------------------------------------------------------------------------------------
// the tile of one chain's next term from its accumulator: term buffer, running sum (workspace), the two norms
template <int NP>
__device__ __forceinline__ void lind_hvp_commit(const d4 &cr, const d4 &ci, const double fac, lind_gd *Y, lind_gd *S, const unsigned (&o)[4],
                                                double &t2, double &s2) {
    constexpr int NP2 = NP * NP;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double ur = fac * cr[r], ui = fac * ci[r];
        Y[o[r]] = ur; Y[NP2 + o[r]] = ui;
        const double vr = S[o[r]] + ur, vi = S[NP2 + o[r]] + ui;
        S[o[r]] = vr; S[NP2 + o[r]] = vi;
        t2 += ur * ur + ui * ui;
        s2 += vr * vr + vi * vi;
    }
}

// lind_tile with opaque lane offsets: the compiler redoes the address arithmetic of a section where the section uses it.
// Otherwise it keeps a lane offset per (buffer, plane, element) of every section alive across the whole time loop, and the
// NP = 48 and 64 instantiations spill.
template <int NP>
__device__ __forceinline__ LindTile lind_hvp_tile(const int tile, const int lane) {
    LindTile g = lind_tile<NP>(tile, lane);
    asm volatile("" : "+v"(g.aoff), "+v"(g.boff), "+v"(g.o[0]), "+v"(g.o[1]), "+v"(g.o[2]), "+v"(g.o[3]));
    return g;
}

template <int NP>
__global__ void __launch_bounds__(LindBwd<NP>::NTH) lind_hvp_backward_kernel(LindHvpArgs q) {
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

    {   // chi_k(T) = c_k sigma_k (the coefficients of lind_backward_kernel, not normalised), chi'_k(T) = c'_k sigma_k
        double cfr = 0., cfi = 0.;
        const double w = a.weights ? a.weights[k] : 1.0, Kt = (double)a.K_total;
        if (a.functional == 0) { cfr = w * a.f[0] / (Kt * Kt); cfi = w * a.f[1] / (Kt * Kt); }
        else if (a.functional == 1) { const double2 t = a.tau[k]; cfr = w * t.x / Kt; cfi = w * t.y / Kt; }
        else { cfr = w / (2.0 * Kt); }
        const double2 dc = q.dcoef[wd];
        const lind_gd *sg = lind_uniform(a.target + (size_t)k * 2 * NP2);
        lind_gd *C0 = lind_uniform(Cb), *Cp0 = lind_uniform(Cpb);
        for (int t = 0; t < TPW; ++t) {
            const LindTile g = lind_hvp_tile<NP>(wave * TPW + t, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double tr = sg[g.o[r]], tim = sg[NP2 + g.o[r]];
                const double vr = cfr * tr - cfi * tim, vi = cfr * tim + cfi * tr;
                const double wr = dc.x * tr - dc.y * tim, wi = dc.x * tim + dc.y * tr;
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
