// grape_expect.hip.h -- expectation values of operator observables on the stored forward states (grape_expect).
//
// The reference lets a trajectory carry `observables` through its forward sweep: cb(propagator, observables) after every
// prop_step! (src/optimize.jl:733-737 of the reference).  Here the sweep has already run and its states are on the device:
//   closed handle   e[k][n][m] = <Psi_k(t_n)| O_m |Psi_k(t_n)>     store [K][N_T+1][NP] interleaved (every route)
//   open handle     e[k][n][m] = tr(O_m rho_k(t_n))                store [K][N_T+1][2][NP*NP] planar row-major
// Nothing here is translated from the reference (which has no kernels).  Both kernels only read the store; they write a
// result buffer of their own.  No atomics, no scratch, every sum in a fixed order that does not depend on M or on the position
// of an operator in the set: the m loop is one piece of code run M times, nothing is carried from one observable to the next.
#pragma once
#include "grape_kernels.hip.h"

// ---------------------------------------------------------------------------------------
// Closed handles: Y = O Phi on the matrix pipe, then the column-wise Phi^dagger . Y.
//
// grid (ceil((N_T+1) / 16), K), 256 threads.  The 16 stored states of a block are the NP x 16 right-hand operand, in the LDS as
// X[row][time] (two planes).  Rows >= N and grid points > N_T are written as zeros whatever the store holds there: no route's
// padding is relied on.  Wave w owns the 16-row tiles w, w + 4, ... of Y; the k loop runs in steps of 4 with four real
// v_mfma_f64_16x16x4f64 per complex step.  The operator comes in the order the lanes consume it (expect_pack_closed on the
// host): one 512-byte line per wave load.  Accumulator element (row = 16 ti + (lane >> 4) + 4 r, time = lane & 15) is
// multiplied by conj Phi[row][time] in the lane that holds it; rows are summed in the lane (r, then ti), across the four lane
// groups of a column (xor 16, xor 32), across the waves through the LDS in wave order.
// ---------------------------------------------------------------------------------------
struct ExpectArgs {
    const double2 *fw;   // [K][N_T+1][NP]
    const double *ops;   // [Ko][M][NP/16][NP/4][2][64] fragments of the zero-padded (balanced) operators
    size_t stride_k;     // doubles between the operator sets of two trajectories (0: one set for all)
    double2 *out;        // [K][N_T+1][M]
    int N, NP, N_T, M;
};

constexpr int EXPECT_NTH = 256;
inline size_t expect_lds_bytes(int NP) { return ((size_t)2 * NP * 16 + 2 * 4 * 32) * sizeof(double); }

__global__ void __launch_bounds__(EXPECT_NTH) expect_closed_kernel(ExpectArgs a) {
    extern __shared__ double ex_lds[];
    const int NP = a.NP, NT = NP >> 4, KS = NP >> 2;   // (NP is a multiple of 16)
    double *Xr = ex_lds, *Xi = ex_lds + NP * 16, *red = ex_lds + 2 * NP * 16;   // red[2][4 waves][16 times][re, im]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lg = lane >> 4;
    const int k = blockIdx.y, n0 = 16 * blockIdx.x;
    const double2 *src = a.fw + ((size_t)k * (a.N_T + 1) + n0) * NP;
    for (int idx = tid; idx < 16 * NP; idx += EXPECT_NTH) {
        const int t = idx & 15, row = idx >> 4;
        double2 v = make_double2(0., 0.);
        if (n0 + t <= a.N_T && row < a.N) v = src[(size_t)t * NP + row];
        Xr[idx] = v.x; Xi[idx] = v.y;
    }
    __syncthreads();
    const double *Ok = a.ops + (size_t)k * a.stride_k;
#pragma unroll 1
    for (int m = 0; m < a.M; ++m) {
        const double *Om = Ok + (size_t)m * 2 * NP * NP;
        double sr = 0., si = 0.;
        for (int ti = wave; ti < NT; ti += 4) {
            d4 cr = {0., 0., 0., 0.}, ci = {0., 0., 0., 0.};
            const double *f = Om + (size_t)ti * KS * 128 + lane;
            unsigned bo = (unsigned)(lg * 16 + lc);
            for (int k4 = 0; k4 < NT; ++k4) {   // (NP / 4 = 4 NT slices, four at a time)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double ar = f[128 * q], ai = f[128 * q + 64];
                    const double br = Xr[bo + 64 * q], bi = Xi[bo + 64 * q];
                    cr = MFMA64(ar, br, cr);
                    ci = MFMA64(ar, bi, ci);
                    cr = MFMA64(-ai, bi, cr);
                    ci = MFMA64(ai, br, ci);
                }
                f += 512; bo += 256;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned po = (unsigned)((16 * ti + lg + 4 * r) * 16 + lc);
                const double pr = Xr[po], pi = Xi[po];
                sr += pr * cr[r] + pi * ci[r];
                si += pr * ci[r] - pi * cr[r];
            }
        }
        sr += __shfl_xor(sr, 16); si += __shfl_xor(si, 16);
        sr += __shfl_xor(sr, 32); si += __shfl_xor(si, 32);
        double *rm = red + (m & 1) * 128;   // (two buffers: one barrier per observable)
        if (lane < 16) { rm[wave * 32 + 2 * lane] = sr; rm[wave * 32 + 2 * lane + 1] = si; }
        __syncthreads();
        if (tid < 32) {
            const double v = ((rm[tid] + rm[32 + tid]) + rm[64 + tid]) + rm[96 + tid];
            const int n = n0 + (tid >> 1);
            if (n <= a.N_T) ((double *)a.out)[2 * (((size_t)k * (a.N_T + 1) + n) * a.M + m) + (tid & 1)] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Open handles: tr(O rho) = sum_ij O_ij rho_ji, element-wise on the planar store.
//
// grid K (N_T + 1), 256 threads: one workgroup per stored state.  The state is read once, as double2, into registers (elements
// of the padding are replaced by zeros); every operator -- uploaded transposed, W[i NP + j] = O_ji, so that it is read in the
// order of the store -- is then multiplied against it: strided partial sums per thread in index order, a wave butterfly, the
// four waves through the LDS in wave order.
// ---------------------------------------------------------------------------------------
struct ExpectOpenArgs {
    const double *store;   // [K][N_T+1][2][NP*NP]
    const double *ops;     // [Ko][M][2][NP*NP] planar, transposed, zero padded
    size_t stride_k;       // doubles: 0 or M 2 NP^2
    double2 *out;          // [K][N_T+1][M]
    int N, N_T, M;
};

template <int NP>
__global__ void __launch_bounds__(EXPECT_NTH) expect_open_kernel(ExpectOpenArgs a) {
    constexpr int NP2 = NP * NP, PAIRS = NP2 / 2, PER = (PAIRS + EXPECT_NTH - 1) / EXPECT_NTH;
    __shared__ double red[2][4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cell = blockIdx.x;   // k (N_T + 1) + n
    const int k = (int)(cell / (size_t)(a.N_T + 1));
    const double2 *sr = (const double2 *)(a.store + cell * 2 * NP2), *si = sr + PAIRS;
    double2 xr[PER], xi[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int p = tid + q * EXPECT_NTH;
        xr[q] = make_double2(0., 0.); xi[q] = make_double2(0., 0.);
        if (p < PAIRS) {
            const int i = (2 * p) / NP, j = (2 * p) % NP;   // (NP is even: both elements of a pair are in row i)
            const double2 vr = sr[p], vi = si[p];
            if (i < a.N && j < a.N) { xr[q].x = vr.x; xi[q].x = vi.x; }
            if (i < a.N && j + 1 < a.N) { xr[q].y = vr.y; xi[q].y = vi.y; }
        }
    }
    const double *Ok = a.ops + (size_t)k * a.stride_k;
#pragma unroll 1
    for (int m = 0; m < a.M; ++m) {
        const double2 *wr = (const double2 *)(Ok + (size_t)m * 2 * NP2), *wi = wr + PAIRS;
        double er = 0., ei = 0.;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int p = tid + q * EXPECT_NTH;
            if (p < PAIRS) {
                const double2 or_ = wr[p], oi = wi[p];
                er += or_.x * xr[q].x - oi.x * xi[q].x;
                ei += or_.x * xi[q].x + oi.x * xr[q].x;
                er += or_.y * xr[q].y - oi.y * xi[q].y;
                ei += or_.y * xi[q].y + oi.y * xr[q].y;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { er += __shfl_xor(er, off); ei += __shfl_xor(ei, off); }
        if (lane == 0) { red[m & 1][wave][0] = er; red[m & 1][wave][1] = ei; }
        __syncthreads();
        if (tid < 2)
            ((double *)a.out)[2 * (cell * a.M + m) + tid] = ((red[m & 1][0][tid] + red[m & 1][1][tid]) + red[m & 1][2][tid]) + red[m & 1][3][tid];
    }
}

// ---- host side of the layouts ----

// O [N*N] complex column-major (the ABI) -> fragments [NP/16][NP/4][2][64] of the zero-padded D O D (bal: D = diag(2^e) of a
// balanced handle, exact; nullptr: the identity).  Lane l of tile (ti, ks) holds O[16 ti + (l & 15)][4 ks + (l >> 4)].
inline void expect_pack_closed(const double *src, int N, int NP, const double *bal, double *dst) {
    const int KS = NP / 4;
    for (int ti = 0; ti < NP / 16; ++ti)
        for (int ks = 0; ks < KS; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int i = 16 * ti + (l & 15), j = 4 * ks + (l >> 4);
                double re = 0., im = 0.;
                if (i < N && j < N) {
                    const double f = bal ? bal[i] * bal[j] : 1.0;
                    re = f * src[2 * ((size_t)j * N + i)]; im = f * src[2 * ((size_t)j * N + i) + 1];
                }
                double *d = dst + ((size_t)ti * KS + ks) * 128;
                d[l] = re; d[64 + l] = im;
            }
}

// O [N*N] complex column-major -> planar row-major transpose W[i NP + j] = O_ji, zero padded: src[2 (i N + j)] is O_ji
inline void expect_pack_open(const double *src, int N, int NP, double *dst) {
    const size_t np2 = (size_t)NP * NP;
    for (size_t e = 0; e < 2 * np2; ++e) dst[e] = 0.;
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            dst[(size_t)i * NP + j] = src[2 * ((size_t)i * N + j)];
            dst[np2 + (size_t)i * NP + j] = src[2 * ((size_t)i * N + j) + 1];
        }
}
