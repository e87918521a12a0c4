// Trace tables of the generator classes: tr H^8, tr H^6 and -- for the segment certificate -- tr H^4, tr H^12 as polynomials
// in the pulse values.
//
// The four-product cell (asm/gen_t16.py) certifies its spectrum by m8 = dt^8 tr H^8 <= theta^8 and m6 = dt^6 tr H^6 >= 0,
// H = H0_k + sum_l e_l C_l.  Both traces are polynomials in e = (e_1 .. e_L) whose coefficients depend on the operators
// alone, so t16_plan_kernel (grape_kernels.hip.h) can decide the same inequality -- with a wider margin -- from the
// pulse values before the launch, and a cell it certifies skips the in-cell bound.  From m4, m8 and m12 the same kernel
// certifies a cell for the segment of the shortest economized derivative series (t16_seg_certified).  Built once per handle,
// next to the Gram matrices, on the device, in plain HIP C++ (not on the timed path):
//
//     H   = sum_a x_a O_a,  x_0 = 1, x_l = e_l,  O = (H0_k, C_1 .. C_L)         M = L + 1 variables, homogeneous
//     H^2 = sum_|al|=2 x^al M2_al      M2_(a)+(b) += O_a O_b   (ordered products)
//     H^3 = H^2 H,  H^4 = H^2 H^2      M3_al+(c) += M2_al O_c,  M4_al+be += M2_al M2_be
//     t8[al + be] += Re tr(M4_al M4_be),   t6[al + be] += Re tr(M3_al M3_be)
//     H^6 = H^3 H^3                    M6_al+be += M3_al M3_be                              (segment tables only)
//     t4[al + be] += Re tr(M2_al M2_be),   t12[al + be] += Re tr(M6_al M6_be)
//
// At L = 2: 6 + 10 + 15 coefficient matrices from 9 + 18 + 36 products, 45 + 28 coefficients per class; with the segment
// tables 28 more matrices from 100 products and 15 + 91 coefficients.  Every sum runs in a fixed order (no atomics): the same
// operators give the same table, whichever of the two sets is built.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <vector>

#define GRAPE_CERT_LMAX 4

// exponent tuples of the monomials of degree d in M variables, 4 bits per variable (variable a at bits 4a), in
// lexicographic order of (alpha_0, alpha_1, ..)
struct CertMonomials {
    std::vector<uint32_t> key;
    std::map<uint32_t, int> index;
    CertMonomials(int M, int d) {
        gen(M, d, 0, 0u);
        for (size_t i = 0; i < key.size(); ++i) index[key[i]] = (int)i;
    }
    int size() const { return (int)key.size(); }

private:
    void gen(int M, int left, int a, uint32_t k) {
        if (a == M - 1) { key.push_back(k | ((uint32_t)left << (4 * a))); return; }
        for (int e = left; e >= 0; --e) gen(M, left - e, a + 1, k | ((uint32_t)e << (4 * a)));
    }
};

// a list of sums  dst[i] = sum over pairs (a, b) of  f(src[a], src[b]):  rows in CSR form
struct CertJobs {
    std::vector<int> row, pair;   // row[i] .. row[i + 1]: the pairs of destination i (2 ints each)
    void from(const std::vector<std::vector<int>> &lists) {
        row.assign(1, 0);
        pair.clear();
        for (const auto &l : lists) {
            pair.insert(pair.end(), l.begin(), l.end());
            row.push_back((int)pair.size() / 2);
        }
    }
};

// the jobs of the tables (they depend on L alone); seg: those of the segment tables as well (M6, t4, t12)
struct CertPlan {
    int M, n2, n3, n4, n6, n8, n12, nmat;   // nmat = M + n2 + n3 + n4 (+ n6) matrices of scratch per class
    CertJobs mm2, mm34, mm6, tr;            // products: M2 | M3 and M4 | M6; traces: t8 | t6 | t4 | t12
    std::vector<int> exps;                  // [n8 + n6 (+ n4 + n12)] exponents of e_1 .. e_L of every coefficient, 4 bits each
    explicit CertPlan(int L, bool seg = false) {
        M = L + 1;
        const CertMonomials m2(M, 2), m3(M, 3), m4(M, 4), m6(M, 6), m8(M, 8), m12(M, 12);
        n2 = m2.size(); n3 = m3.size(); n4 = m4.size(); n6 = m6.size(); n8 = m8.size(); n12 = seg ? m12.size() : 0;
        const int o2 = M, o3 = o2 + n2, o4 = o3 + n3, o6 = o4 + n4;
        nmat = o6 + (seg ? n6 : 0);
        auto var = [&](int a) { return (uint32_t)1 << (4 * a); };   // (sums of keys never carry: the degrees stay <= 12)
        std::vector<std::vector<int>> l2(n2), l34(n3 + n4), l6(seg ? n6 : 0), lt(n8 + n6 + (seg ? n4 + n12 : 0));
        for (int a = 0; a < M; ++a)
            for (int b = 0; b < M; ++b) { auto &l = l2[m2.index.at(var(a) + var(b))]; l.push_back(a); l.push_back(b); }
        for (int i = 0; i < n2; ++i)
            for (int c = 0; c < M; ++c) { auto &l = l34[m3.index.at(m2.key[i] + var(c))]; l.push_back(o2 + i); l.push_back(c); }
        for (int i = 0; i < n2; ++i)
            for (int j = 0; j < n2; ++j) { auto &l = l34[n3 + m4.index.at(m2.key[i] + m2.key[j])]; l.push_back(o2 + i); l.push_back(o2 + j); }
        for (int i = 0; i < n4; ++i)
            for (int j = 0; j < n4; ++j) { auto &l = lt[m8.index.at(m4.key[i] + m4.key[j])]; l.push_back(o4 + i); l.push_back(o4 + j); }
        for (int i = 0; i < n3; ++i)
            for (int j = 0; j < n3; ++j) { auto &l = lt[n8 + m6.index.at(m3.key[i] + m3.key[j])]; l.push_back(o3 + i); l.push_back(o3 + j); }
        if (seg) {
            for (int i = 0; i < n3; ++i)
                for (int j = 0; j < n3; ++j) { auto &l = l6[m6.index.at(m3.key[i] + m3.key[j])]; l.push_back(o3 + i); l.push_back(o3 + j); }
            for (int i = 0; i < n2; ++i)
                for (int j = 0; j < n2; ++j) { auto &l = lt[n8 + n6 + m4.index.at(m2.key[i] + m2.key[j])]; l.push_back(o2 + i); l.push_back(o2 + j); }
            for (int i = 0; i < n6; ++i)
                for (int j = 0; j < n6; ++j) { auto &l = lt[n8 + n6 + n4 + m12.index.at(m6.key[i] + m6.key[j])]; l.push_back(o6 + i); l.push_back(o6 + j); }
        }
        mm2.from(l2); mm34.from(l34); mm6.from(l6); tr.from(lt);
        for (int i = 0; i < n8; ++i) exps.push_back((int)(m8.key[i] >> 4));
        for (int i = 0; i < n6; ++i) exps.push_back((int)(m6.key[i] >> 4));
        if (seg) {
            for (int i = 0; i < n4; ++i) exps.push_back((int)(m4.key[i] >> 4));
            for (int i = 0; i < n12; ++i) exps.push_back((int)(m12.key[i] >> 4));
        }
    }
};

// operators of the classes of a chunk, planar row-major with row length NP -> scratch matrices 0 .. M - 1 (row-major N x N)
__global__ void __launch_bounds__(256) cert_load_kernel(const double *H0f, const double *Hcf, const int *rep, int kc0, int hc_per_traj, int L,
                                                        int N, int NP, int nmat, double2 *scratch) {
    const int a = blockIdx.x, c = blockIdx.y, kc = kc0 + c, k = rep ? rep[kc] : kc;
    const size_t pp = (size_t)NP * NP;
    const double *src = a == 0 ? H0f + (size_t)k * 2 * pp : Hcf + ((size_t)(hc_per_traj ? k : 0) * L + (a - 1)) * 2 * pp;
    double2 *dst = scratch + ((size_t)c * nmat + a) * N * N;
    for (int e = threadIdx.x; e < N * N; e += 256) {
        const int i = e / N, j = e - i * N;
        dst[e] = make_double2(src[(size_t)i * NP + j], src[pp + (size_t)i * NP + j]);
    }
}

// scratch[dst0 + blockIdx.x] = sum over its pairs (a, b) of scratch[a] scratch[b] (complex N x N), class blockIdx.y
__global__ void __launch_bounds__(256) cert_mm_kernel(double2 *scratch, int nmat, int N, int dst0, const int *row, const int *pair) {
    double2 *base = scratch + (size_t)blockIdx.y * nmat * N * N;
    double2 *dst = base + (size_t)(dst0 + blockIdx.x) * N * N;
    const int p0 = row[blockIdx.x], p1 = row[blockIdx.x + 1];
    for (int e = threadIdx.x; e < N * N; e += 256) {
        const int i = e / N, j = e - i * N;
        double sr = 0., si = 0.;
        for (int q = p0; q < p1; ++q) {
            const double2 *A = base + (size_t)pair[2 * q] * N * N + (size_t)i * N, *B = base + (size_t)pair[2 * q + 1] * N * N + j;
            double tr = 0., ti = 0.;
            for (int k = 0; k < N; ++k) {
                const double2 x = A[k], y = B[(size_t)k * N];
                tr += x.x * y.x - x.y * y.y;
                ti += x.x * y.y + x.y * y.x;
            }
            sr += tr; si += ti;
        }
        dst[e] = make_double2(sr, si);
    }
}

// table[class][blockIdx.x] = sum over its pairs (a, b) of Re tr(scratch[a] scratch[b])
__global__ void __launch_bounds__(256) cert_trace_kernel(const double2 *scratch, int nmat, int N, const int *row, const int *pair, int nt,
                                                         double *table) {
    __shared__ double red[256];
    const double2 *base = scratch + (size_t)blockIdx.y * nmat * N * N;
    const int p0 = row[blockIdx.x], p1 = row[blockIdx.x + 1];
    double sum = 0.;
    for (int q = p0; q < p1; ++q) {
        const double2 *A = base + (size_t)pair[2 * q] * N * N, *B = base + (size_t)pair[2 * q + 1] * N * N;
        double t = 0.;
        for (int e = threadIdx.x; e < N * N; e += 256) {
            const int i = e / N, j = e - i * N;
            const double2 x = A[e], y = B[(size_t)j * N + i];
            t += x.x * y.x - x.y * y.y;
        }
        sum += t;
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) table[(size_t)blockIdx.y * nt + blockIdx.x] = red[0];
}
