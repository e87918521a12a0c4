// grape_lindblad.hip.h -- open-system GRAPE: d x d density matrices under a Lindblad generator, in matrix form (d <= 64).
//
// The reference treats open systems as first class: the state is a vectorised density matrix, the generator a Liouvillian
// super-operator (docs/src/background.md:46, :240-242).  Handing the d^2 x d^2 Liouvillian to the closed path works up to
// d = 22; this file keeps the structure instead.  On interval n of trajectory k
//     H_eff = H_kn - (i/2) sum_j A_j^dagger A_j,          M = -i H_eff
//     L(X)        = M X + X M^dagger + sum_j (A_j X) A_j^dagger                     (d rho / dt = L(rho))
//     L^dagger(Y) = M^dagger Y + Y M + sum_j (A_j^dagger Y) A_j                     (adjoint for <<Y|X>> = tr(Y^dagger X))
//     (dL/d eps_l)^dagger (Y) = s_ln (D_l^dagger Y + Y D_l),   D_l = -i H_l
// are 2 + 2J products of d x d matrices, each of them a complex GEMM on v_mfma_f64_16x16x4_f64 tiles.
//   forward : rho_n = sum_a u_a,  u_0 = rho_{n-1},  u_{a+1} = dt / (a+1) L(u_a), until ||u_a||_F <= tol ||sum||_F
//   backward: the block recursion of taylor_grad_step! (src/optimize.jl:604-653) on the adjoint side, taken to convergence
//             (what GRAPE_GRAD_GRADGEN promises): c_0 = chi_n, p_0 = 0,
//                 c_{a+1} = dt / (a+1) L^dagger c_a,      p_{a+1} = dt / (a+1) (L^dagger p_a + (dL/d eps_l)^dagger c_a),
//             chi_{n-1} = sum_a c_a,   tau_grads[k][l][n] = rho_k <<sum_a p_a | rho_k(t_n)>>.
//   Long steps are cut into m = ceil(beta_n dt_n / theta) sub-steps, beta_n = 2 (r0_k + sum_l |s eps| r_l) + sum_j ||A_j||^2
//   >= ||L_kn|| from norm estimates made at create time.  The pair (p, c) is propagated by the exponential of the block
//   generator [[L^dagger, dL^dagger], [0, L^dagger]], so a sub-step simply starts from the (p, c) the previous one left:
//   the product rule across the sub-steps is the semigroup property of that exponential.
//
// Layout on the chip.  One workgroup per trajectory walks the forward recurrence (serial in n); the backward launch is a
// grid (K, L) in which every workgroup recomputes the c chain of its trajectory and carries the p chain of ONE control, so
// the serial length of a step is two series whatever L.  A workgroup has one wave per 16 x 16 output tile ((NP / 16)^2 waves:
// 1, 4, 9, 16 at NP = 16, 32, 48, 64); the running sums stay in the registers of the wave that owns the tile, all other
// matrices (M, M^dagger of the step, the two term buffers, the J scratch products A_j X) live in a per-workgroup
// workspace in device memory that stays in the L2 / vector L1, and the MFMA operands are fetched from there directly:
// planar (re plane | im plane) row-major NP x NP, zero padded.  Reductions (norms, overlaps) have a fixed order: wave
// butterfly, then the waves in index order -- results are bitwise repeatable.  No scratch memory, 1 KB of LDS.
#pragma once
#include "grape_kernels.hip.h"
#include "grape_series.hip.h"   // c_series_inv

#define LIND_MAX_J 8
#define LIND_MAX_ORDER 200

struct LindArgs {
    const double *H0;       // [K][2][NP*NP] drift
    const double *Hc;       // [Kc][L][2][NP*NP] control operators
    const double *Dc;       // [Kc][L][2][2][NP*NP]: D_l = -i H_l, then D_l^dagger (backward only)
    const double *A;        // [Kj][J][2][2][NP*NP]: A_j, then A_j^dagger
    const double *AdA;      // [Kj][2][NP*NP]: sum_j A_j^dagger A_j (zero for J = 0)
    const double *rho0;     // [K][2][NP*NP] initial states
    const double *target;   // [K][2][NP*NP] targets sigma_k
    const double *chi_in;   // nullptr or [K][2][NP*NP]: the caller's chi_k(T) (grape_backward_chi)
    const double *weights;  // nullptr or [K]
    const double *eps, *shape, *dts;
    const double *rb;       // [K] r0_k | [Kc][L] r_l | [Kj] sum_j ||A_j||_2^2   (2-norm estimates)
    double *store;          // [K][N_T+1][2][NP*NP] rho_k(t_n)
    double *ws;             // per-workgroup workspace
    double2 *tau;           // [K] forward: out, backward: in
    const double *f;        // [2] all-reduced sum_k w_k tau_k
    double *rho;            // [K] ||chi_k(T)||_F
    double2 *tg;            // [K][L][N_T] tau_grads
    int *flags;             // [0] |= 2: chi norm guard, |= 16: a series did not converge
    unsigned long long *stats;   // [workgroup][2]: series terms, (sub-)steps
    double tol, theta, chi_min_norm;
    int K, K_total, L, J, N_T, functional, hc_per_traj, cops_per_traj;
};

// Every matrix of a workgroup has a uniform base address.  Pinning it to scalar registers makes an element access base +
// 32-bit lane offset; otherwise the compiler keeps a 64-bit lane address per (matrix, element) alive across the time loop
// and the NP = 64 kernels (16 waves, 128 registers per lane) spill.
typedef __attribute__((address_space(1))) double lind_gd;   // (the pinned pointer keeps its address space: global, not flat, loads)
__device__ __forceinline__ lind_gd *lind_uniform(double *p) {
    asm volatile("" : "+s"(p));
    return (lind_gd *)p;
}
__device__ __forceinline__ const lind_gd *lind_uniform(const double *p) {
    asm volatile("" : "+s"(p));
    return (const lind_gd *)p;
}
__device__ __forceinline__ lind_gd *lind_uniform(lind_gd *p) {
    asm volatile("" : "+s"(p));
    return p;
}

// acc += Lf * Rt on one 16 x 16 tile: Lf, Rt planar row-major in device memory, aoff / boff the lane's operand offsets
// (A operand: row 16 ti + lane % 16, k = 4 ks + lane / 16; B operand: k = 4 ks + lane / 16, column 16 tj + lane % 16)
template <int NP>
__device__ __forceinline__ void lind_mac(d4 &cr, d4 &ci, const double *Lf, const double *Rt, const unsigned aoff, const unsigned boff) {
    constexpr int NP2 = NP * NP;
    // the four plane bases are uniform: pinned to scalar registers here, so that a load is base + 32-bit lane offset and the
    // compiler does not keep a 64-bit lane address per operand of the kernel alive across the whole time loop (spills at NP = 64)
    const lind_gd *lr = lind_uniform(Lf), *li = lind_uniform(Lf + NP2), *rr = lind_uniform(Rt), *ri = lind_uniform(Rt + NP2);
    unsigned ao = aoff, bo = boff;
#pragma unroll 4
    for (int ks = 0; ks < NP / 4; ++ks) {
        const double ar = lr[ao], ai = li[ao];
        const double br = rr[bo], bi = ri[bo];
        ao += 4; bo += 4 * NP;
        cr = MFMA64(ar, br, cr);
        ci = MFMA64(ar, bi, ci);
        cr = MFMA64(-ai, bi, cr);
        ci = MFMA64(ai, br, ci);
    }
}

// the wave's tile of T_j = Al_j X for every j (Al_j at stride 4 NP^2: the A_j / A_j^dagger pairs of LindArgs::A)
template <int NP>
__device__ __forceinline__ void lind_left_products(double *Tm, const double *Al, const double *X, const int J, const unsigned aoff,
                                                   const unsigned boff, const unsigned (&o)[4]) {
    constexpr int NP2 = NP * NP;
    for (int j = 0; j < J; ++j) {
        d4 cr = (d4){0., 0., 0., 0.}, ci = (d4){0., 0., 0., 0.};
        lind_mac<NP>(cr, ci, Al + (size_t)j * 4 * NP2, X, aoff, boff);
        lind_gd *t = lind_uniform(Tm + (size_t)j * 2 * NP2);
#pragma unroll
        for (int r = 0; r < 4; ++r) { t[o[r]] = cr[r]; t[NP2 + o[r]] = ci[r]; }
    }
}

// acc += P X + X Pd + sum_j T_j Ar_j
template <int NP>
__device__ __forceinline__ void lind_apply_tile(d4 &cr, d4 &ci, const double *P, const double *Pd, const double *X, const double *Tm,
                                                const double *Ar, const int J, const unsigned aoff, const unsigned boff) {
    constexpr int NP2 = NP * NP;
    lind_mac<NP>(cr, ci, P, X, aoff, boff);
    lind_mac<NP>(cr, ci, X, Pd, aoff, boff);
    for (int j = 0; j < J; ++j) lind_mac<NP>(cr, ci, Tm + (size_t)j * 2 * NP2, Ar + (size_t)j * 4 * NP2, aoff, boff);
}

// M = -i (H0_k + sum_l e_l H_l) - 1/2 sum_j A_j^dagger A_j and M^dagger of interval n; returns beta_n (every thread the same)
template <int NP, int NTH>
__device__ __forceinline__ double lind_build_generator(const LindArgs &a, const int k, const int n, double *M, double *Md) {
    constexpr int NP2 = NP * NP;
    const int L = a.L, N_T = a.N_T, Kc = a.hc_per_traj ? a.K : 1, kc = a.hc_per_traj ? k : 0, kj = a.cops_per_traj ? k : 0;
    const lind_gd *H0 = lind_uniform(a.H0 + (size_t)k * 2 * NP2), *AdA = lind_uniform(a.AdA + (size_t)kj * 2 * NP2);
    const double *Hc = a.Hc + (size_t)kc * L * 2 * NP2;
    lind_gd *Mg = lind_uniform(M), *Mdg = lind_uniform(Md);
    double bound = a.rb[k];
    for (int l = 0; l < L; ++l)
        bound += fabs(a.eps[(size_t)l * N_T + n] * (a.shape ? a.shape[(size_t)l * N_T + n] : 1.0)) * a.rb[a.K + kc * L + l];
    for (unsigned idx = threadIdx.x; idx < (unsigned)NP2; idx += NTH) {
        double hr = H0[idx], hi = H0[NP2 + idx];
        for (int l = 0; l < L; ++l) {
            const double e = a.eps[(size_t)l * N_T + n] * (a.shape ? a.shape[(size_t)l * N_T + n] : 1.0);
            const lind_gd *hl = lind_uniform(Hc + (size_t)l * 2 * NP2);
            hr = fma(e, hl[idx], hr);
            hi = fma(e, hl[NP2 + idx], hi);
        }
        const double mr = hi - 0.5 * AdA[idx], mi = -hr - 0.5 * AdA[NP2 + idx];
        const unsigned i = idx / NP, j = idx - i * NP;
        Mg[idx] = mr; Mg[NP2 + idx] = mi;
        Mdg[j * NP + i] = mr; Mdg[NP2 + j * NP + i] = -mi;
    }
    return 2.0 * bound + a.rb[a.K + Kc * L + kj];
}

__device__ __forceinline__ int lind_substeps(const double beta, const double dt, const double theta) {
    const int m = (int)ceil(beta * dt / theta);
    return m < 1 ? 1 : (m > 4096 ? 4096 : m);   // (NaN: 1)
}

// ---------------------------------------------------------------------------------------
// Forward sweep: grid K, one workgroup per trajectory.  Workspace per workgroup: M | M^dagger | U[2] | T[J].
// ---------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(NP * NP / 4) lind_forward_kernel(LindArgs a) {
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

// ---------------------------------------------------------------------------------------
// Backward sweep and gradient: grid (K, L).  Workspace per workgroup: M | M^dagger | C[2] | P[2] | sum C | sum P | Tc[J] | Tp[J].
// Two chains and the derivative term need more registers than the 128 per lane that 16 waves leave: at NP = 64 a wave owns
// two tiles and works through them one after the other (8 waves), and the running sums stay in the workspace (every lane
// updates its own elements).
// ---------------------------------------------------------------------------------------
template <int NP>
struct LindBwd {
    static constexpr int T = NP / 16, TPW = NP == 64 ? 2 : 1, NW = T * T / TPW, NTH = 64 * NW;
};

struct LindTile {
    unsigned aoff, boff, o[4];
};
template <int NP>
__device__ __forceinline__ LindTile lind_tile(const int tile, const int lane) {
    constexpr int T = NP / 16;
    const int ti = tile / T, tj = tile - ti * T;
    LindTile g;
    g.aoff = (16 * ti + (lane & 15)) * NP + (lane >> 4);
    g.boff = (lane >> 4) * NP + 16 * tj + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) g.o[r] = (16 * ti + 4 * r + (lane >> 4)) * NP + 16 * tj + (lane & 15);
    return g;
}

template <int NP>
__global__ void __launch_bounds__(LindBwd<NP>::NTH) lind_backward_kernel(LindArgs a) {
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
