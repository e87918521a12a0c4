// grape_batch.hip.h -- many pulse vectors through the problem of one handle (grape_eval_batch).
//
// Multi-start optimisation, a population of optimisers, the trial points of a line search: all of them evaluate the SAME
// problem at DIFFERENT pulsevals, and for a small system (N <= 16, few trajectories) each of those evaluations is a
// latency-bound chain on an idle chip.  Here the pulse set is one more grid axis: blockIdx.y = p selects the set, the
// argument block of the single-set kernel is rebased to the buffers of that set (pulses, propagators, stored states,
// tau_grads, result slab with its flags), and the kernel's own __device__ body runs unchanged on it.  Consequences:
//   - a set computes exactly what the same body computes for it in any other batch: the work distribution inside a set
//     depends on blockIdx.x / gridDim.x only, every reduction (tau sums, chi coefficients, the sum of tau_grads over the
//     trajectories) is segmented over p and keeps the fixed order of the single-set kernel -- a set does not see its
//     neighbours, bit for bit;
//   - the static problem (H0f, Hcf, H0t, Hct, psi0, target, weights, dts, shape, class tables, operator norms) is shared
//     by all sets, nothing is replicated;
//   - with 2 K P one-wave sweeps in flight the chip is full, so the sweeps are the sequential ones (the scan of round 6
//     buys latency with 16 x the flops, which a batch does not need); the backward sweep starts from the unit targets in
//     the same launch as the forward sweep and chi_coeff supplies z_k afterwards, per set;
//   - no launch depends on device data of the batch: H2D of the pulses, the kernels, one D2H of the result slabs.
// The exponential wrapper is compiled in the translation unit of the polynomial kernel (grape_t18.hip defines
// GRAPE_BATCH_T18_UNIT before it includes this file), everything else in grape_hip.hip.
#pragma once
#include <hip/hip_runtime.h>

// element strides from the buffers of one pulse set to those of the next
struct BatchStrides {
    size_t eps;    // doubles: L N_T
    size_t Sf;     // doubles: N_T 2 NP^2 (summed controls of every time step; 0: not used)
    size_t U;      // double2: KC N_T NP^2
    size_t vec;    // double2: K (N_T + 1) NP (forward and backward storage)
    size_t tg;     // double2: K L N_T
    size_t slab;   // doubles, even: [tau (2K) | sums (8) | G (L N_T) | flags (8 ints) | pad]
    size_t k;      // K: rho, z
};

#ifdef GRAPE_BATCH_T18_UNIT

// one wave per cell (p, class, n): the five-product degree-18 polynomial with scaling and squaring of expm_t18_kernel<1>
template <bool CHEB>
__global__ void __launch_bounds__(64) batch_expm_kernel(ExpmArgs a, BatchStrides st) {
    const size_t p = blockIdx.y;
    a.eps += p * st.eps;
    if (a.Sf) a.Sf += p * st.Sf;
    a.U += p * st.U;
    a.flags = (int *)((double *)a.flags + p * st.slab);
    expm_t18_body<1, false, CHEB, false>(a);
}

#else

// S_n = sum_l eps_ln shape_ln H_l of every time step and set (more than two shared controls); grid (N_T, parts, P)
__global__ void __launch_bounds__(256) batch_ctrl_sum_kernel(CtrlSumArgs a, BatchStrides st) {
    const size_t p = blockIdx.z;
    a.eps += p * st.eps;
    a.Sf += p * st.Sf;
    ctrl_sum_body(a);
}

__device__ __forceinline__ void batch_rebase(SweepArgs &a, const BatchStrides &st, const size_t p) {
    a.U += p * st.U;
    a.store += p * st.vec;
    a.tau = (double2 *)((double *)a.tau + p * st.slab);
    a.rho += p * st.k;
    a.flags = (int *)((double *)a.flags + p * st.slab);
}

// one wave per (p, k, direction): grid (2K, P); functional only: batch_sweep_fw_kernel, grid (K, P)
__global__ void __launch_bounds__(64) batch_sweep_pair_kernel(SweepArgs af, SweepArgs ab, BatchStrides st) {
    __shared__ double2 xs[16];
    const size_t p = blockIdx.y;
    if ((int)blockIdx.x < af.K) {
        batch_rebase(af, st, p);
        sweep1w_body<16, false>(af, blockIdx.x, xs);
    } else {
        batch_rebase(ab, st, p);
        sweep1w_body<16, true>(ab, blockIdx.x - af.K, xs);
    }
}
__global__ void __launch_bounds__(64) batch_sweep_fw_kernel(SweepArgs af, BatchStrides st) {
    __shared__ double2 xs[16];
    batch_rebase(af, st, blockIdx.y);
    sweep1w_body<16, false>(af, blockIdx.x, xs);
}

// the partial sums of every set, each in the order of tau_reduce_kernel; grid (1, P), one wave
__global__ void batch_tau_reduce_kernel(double *slab, const double *weights, int K, BatchStrides st) {
    double *out = slab + (size_t)blockIdx.y * st.slab;
    tau_reduce_body((const double2 *)out, weights, K, out + 2 * (size_t)K);
}

// rho_k and z_k of every set from its own sums (f = the first two); grid (ceil(K / 64), P)
__global__ void batch_chi_coeff_kernel(ChiCoeffArgs a, BatchStrides st) {
    const size_t p = blockIdx.y;
    double *slab = (double *)a.s.tau + p * st.slab;
    a.s.tau = (double2 *)slab;
    a.s.f = slab + 2 * (size_t)a.s.K;
    a.s.flags = (int *)((double *)a.s.flags + p * st.slab);
    a.rho += p * st.k;
    a.z += p * st.k;
    chi_coeff_body(a);
}

// derivative overlaps, Taylor sum, sub-stepped where ||H dt|| asks for it (deriv_kernel); grid (blocks of a set, P)
template <int LMAX>
__global__ void __launch_bounds__(DERIV16_NTH) batch_deriv_kernel(DerivArgs a, BatchStrides st) {
    const size_t p = blockIdx.y;
    a.eps += p * st.eps;
    a.fw += p * st.vec;
    a.bw += p * st.vec;
    a.tg += p * st.tg;
    a.flags = (int *)((double *)a.flags + p * st.slab);
    deriv_body<16, LMAX, DERIV16_NTH>(a);
}

// G_p[l N_T + n] = -2 Re sum_k z_pk tau_grads~[p][k][l][n] in the fixed order of grad_reduce_kernel; grid (ceil(L N_T / 16), P)
__global__ void __launch_bounds__(256) batch_grad_reduce_kernel(double2 *tg, int K, int LN, double *slab, const double2 *z, BatchStrides st) {
    const size_t p = blockIdx.y;
    grad_reduce_body(tg + p * st.tg, K, LN, slab + p * st.slab + 2 * (size_t)K + 8, z + p * st.k);
}

#endif
