/*
 * grape_hip.h -- C ABI of the MI355X-native GRAPE gradient evaluator.
 *
 * This is the drop-in boundary for the hot path of JuliaQuantumControl/GRAPE.jl: one call of
 * grape_eval() replaces the body of
 *     evaluate_functional(pulsevals, wrk)        /root/reference/src/optimize.jl:696-768
 *     evaluate_gradient!(G, pulsevals, wrk)      /root/reference/src/optimize.jl:824-1014
 * i.e. what the closure fg!(F, G, pulsevals) (src/optimize.jl:105-111) does when the optimizer
 * backend calls it (ext/GRAPELBFGSBExt.jl:99, ext/GRAPEOptimExt.jl:31), for trajectories whose
 * generator is H_k(t) = H0_k + sum_l eps_l(t) S_l(t) H_l propagated with `prop_method = ExpProp`.
 * grape_create() replaces the data-layout half of the GrapeWrk constructor
 * (/root/reference/src/workspace.jl:147-362): it uploads the static problem and allocates the
 * forward storage (workspace.jl:215), tau_grads (workspace.jl:236-237) and gradient buffers
 * (workspace.jl:196-198) in HBM.
 *
 * Conventions
 *   - plain C, no exceptions, no torch types; every function returns 0 on success or a negative
 *     grape_status; the message of the last failure is available from grape_last_error().  Every entry point is an
 *     exception barrier: a C++ exception raised by the host side (std::bad_alloc of a staging vector, std::system_error
 *     of a shard thread) is caught inside the library, everything the call had allocated is released, and the caller
 *     (a Julia process behind `ccall`) sees GRAPE_ERR_HOST with the exception's message -- never std::terminate.
 *   - complex numbers are interleaved (re, im) doubles == Julia ComplexF64 == C double _Complex.
 *   - matrices are COLUMN-major N x N (Julia Matrix{ComplexF64}); states are length-N vectors.
 *   - pulsevals / G are CONTROL-major: index (l * N_T + n), l < L, n < N_T
 *     (workspace.jl:159-162, optimize.jl:579, 935-936).
 *   - host pointers are owned by the caller and are not retained after the call returns
 *     (they may be Julia-GC managed: `obj.g`, `wrk.pulsevals`).  One in-flight call per handle.
 *   - trajectories may be sharded over processes/GPUs: a handle owns K local trajectories out of
 *     K_total; the two cross-trajectory reductions of the path (sum_k w_k tau_k for J_T_sm/chi_sm,
 *     sum_k of the gradient, optimize.jl:579) are exposed by the split-phase calls below so that
 *     the host can all-reduce them (RCCL) between phases.
 *   - several GPUs behind ONE handle (ABI v4, grape_problem.ndev / .devices): the K trajectories of the
 *     handle are dealt to the devices in contiguous blocks, every host-pointer entry point enqueues the work
 *     of all of them (one host thread per device, asynchronous launches on one stream per device; the
 *     calling thread waits and reads back) and performs the two reductions itself -- RCCL all-reduces on the
 *     shard streams (one communicator rank per device, ncclCommInitAll) when every shard has a device of its
 *     own, otherwise staged through pinned host memory in shard order -- the caller never sees the devices,
 *     exactly like the transparent `@threadsif` loops over k of optimize.jl:720, 876.
 */
#ifndef GRAPE_HIP_H
#define GRAPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRAPE_HIP_ABI_VERSION 7   /* v7 added entry points only: grape_create also accepts abi_version 6 */

typedef struct grape_handle grape_handle;

typedef enum {
    GRAPE_OK = 0,
    GRAPE_ERR_INVALID = -1,      /* bad argument / unsupported size                          */
    GRAPE_ERR_HIP = -2,          /* HIP runtime failure (message has the hipError string)    */
    GRAPE_ERR_CHI_NORM = -3,     /* ||chi_k|| < chi_min_norm          (optimize.jl:1021-1025)*/
    GRAPE_ERR_SINGULAR = -4,     /* Pade denominator numerically singular                    */
    GRAPE_ERR_TAYLOR = -5,       /* Taylor derivative series did not converge (optimize.jl:644-648) */
    GRAPE_ERR_NO_CONTROLS = -6,  /* L == 0                             (workspace.jl:155-157)*/
    GRAPE_ERR_AGAIN = -7,        /* device-pointer API, N > 64 only: the asynchronous launch plan (number of squaring
                                    launches) was too short for this evaluation and has been adapted -- repeat the call.
                                    The host-pointer entry points repeat internally and never return this.          */
    GRAPE_ERR_HOST = -8          /* ABI v6: a host-side C++ exception (out of memory, thread creation) was caught at the
                                    boundary; nothing of the call is left allocated, the handle (if any) stays usable */
} grape_status;

/* J_T of QuantumControl.Functionals (docs/src/tutorial.md:349-356, 402) */
typedef enum {
    GRAPE_J_T_SM = 0,  /* 1 - |sum_k w_k tau_k|^2 / K^2 ; chi_k = w_k (sum_j w_j tau_j) / K^2 * tgt_k */
    GRAPE_J_T_SS = 1,  /* 1 - sum_k w_k |tau_k|^2 / K   ; chi_k = w_k tau_k / K * tgt_k               */
    GRAPE_J_T_RE = 2   /* 1 - Re sum_k w_k tau_k / K    ; chi_k = w_k / (2K) * tgt_k                  */
} grape_functional;

/* gradient_method keyword of the reference (workspace.jl:150, optimize.jl:871-998).
 * GRAPE_GRAD_GRADGEN: the contraction <chi| D exp(-i H dt)[-i dt mu_l] |Psi> to rounding (what the exponential of the gradient
 * generator delivers in the reference), by a two-pass polynomial series on the stored states: the Taylor sum cut at 1e-16,
 * sub-stepped for long steps -- and, for Hermitian cells whose spectrum this evaluation's exponential kernel has certified
 * to lie in a segment of the imaginary axis, the economized polynomial of that segment (same accuracy, fewer orders;
 * DESIGN.md 4.3, tools/econ_coeffs.py; environment GRAPE_DERIV_ECON=0 keeps the Taylor sum everywhere). */
typedef enum {
    GRAPE_GRAD_GRADGEN = 0, /* exact derivative of exp (what the gradient generator yields)  */
    GRAPE_GRAD_TAYLOR = 1   /* Kuprov-Rodgers recursion, taylor_grad_step! (optimize.jl:604) */
} grape_gradient_method;

/* prop_method keyword of the reference (workspace.jl:222-232 -> QuantumPropagators.init_prop) */
typedef enum {
    GRAPE_PROP_EXP = 0,    /* ExpProp: U_n = exp(-i H_n dt_n) materialised on MFMA by an inverse-free polynomial with scaling
                              and squaring: Hermitian generators, 16 < N <= 64 -- degree 16 in four products for the cells
                              whose spectral radius a per-cell bound proves <= 1.36, degree 18 in five products (Chebyshev
                              coefficients, spectral scaling) for the others and for every other size; general matrices
                              -- degree-18 Taylor polynomial.  GRAPE_EXPM_T16=0: five products everywhere;
                              GRAPE_EXPM_T18=0: the order-13 Pade approximant as in Julia's exp! (parity reference).
                              Propagators that do not fit the device make the handle evaluate matrix-free
                              (grape_get_work[12]).                                                                */
    GRAPE_PROP_SERIES = 1  /* matrix-free polynomial propagator on the state vector (the role of the reference's
                              Cheby / Newton methods, README.md:55), no U: N <= 64 power series of exp(-i H_n dt_n) Psi
                              summed to prop_tolerance, O(N^2) per term; 64 < N <= 512 cooperative Chebyshev sweeps
                              (Hermitian generators, guaranteed spectral interval) or Taylor sub-steps              */
} grape_prop_method;

typedef struct {
    int32_t abi_version;     /* GRAPE_HIP_ABI_VERSION                                           */
    int32_t N;               /* Hilbert-space dimension                                         */
    int32_t L;               /* number of controls                                              */
    int32_t K;               /* trajectories owned by this handle (the reference's `N`, :703)   */
    int32_t K_total;         /* trajectories of the whole job (== K when not sharded; 0 => K)   */
    int32_t N_T;             /* time intervals = length(tlist) - 1 (optimize.jl:705)            */
    int32_t functional;      /* grape_functional                                                */
    int32_t gradient_method; /* grape_gradient_method                                           */
    int32_t hc_per_traj;     /* 0: Hc is [L][N*N] shared by all k; 1: Hc is [K][L][N*N]         */
    int32_t device;          /* HIP device ordinal                                              */
    const double *tlist;     /* [N_T+1] time grid (non-uniform allowed)                         */
    const double *H0;        /* [K][N*N] complex: drift of trajectory k                         */
    const double *Hc;        /* control operators mu_l = dH/d eps_l (see hc_per_traj)           */
    const double *shape;     /* NULL or [L][N_T] real: a_l(eps, t_n) = shape[l][n] * eps_{nl}   */
    const double *psi0;      /* [K][N] complex initial states                                   */
    const double *target;    /* [K][N] complex target states.  ABI v6: NULL = trajectories without a target_state
                                (optimize.jl:753: tau_k = NaN) -- legal only with a caller-side J_T / chi pair, i.e.
                                grape_forward + grape_get_final_states + grape_backward_chi / _xi(chi != NULL);
                                grape_eval, grape_backward and the built-in functionals need the targets and refuse */
    const double *weights;   /* NULL (all 1) or [K]                                             */
    double chi_min_norm;     /* <= 0 selects the reference default 1e-100 (optimize.jl:846)     */
    int32_t taylor_max_order;/* <= 0 selects 100   (optimize.jl:915)                            */
    double taylor_tolerance; /* <= 0 selects 1e-16 (optimize.jl:916)                            */
    /* State-dependent running cost of the family g_b(Psi) = <Psi|D|Psi> with xi = -D Psi
     * (optimize.jl:727-750, 764-766, 856-866, 897-908; test/test_state_running_cost.jl:32-40):
     * J gains lambda_b * sum_k trapezoid_n g_b(Psi_k(t_n)), chi the inhomogeneity of
     * docs/src/background.md:771-775.  Dpen == NULL or lambda_b == 0 switches it off.          */
    const double *Dpen;      /* NULL, [N*N] (shared) or [K][N*N] complex Hermitian, column-major */
    int32_t dpen_per_traj;   /* 0: one D for all trajectories; 1: one per trajectory            */
    double lambda_b;
    int32_t prop_method;     /* grape_prop_method (ABI v3)                                      */
    double prop_tolerance;   /* GRAPE_PROP_SERIES: stop at ||term|| < tol ||state||; <= 0 selects 1e-17 */
    /* ABI v4: GPUs behind one handle.  ndev <= 1: the single device `device`.  ndev > 1: trajectory
     * block g (contiguous, sizes differ by at most one) lives on devices[g]; devices == NULL selects
     * device, device+1, ...  An ordinal may repeat (several shards on one GPU).                  */
    int32_t ndev;
    const int32_t *devices;  /* NULL or [ndev] HIP device ordinals                              */
    /* ABI v6: taylor_grad_check_convergence (optimize.jl:917-918, taylor_grad_step! :611, :631-651).  0 = the reference
     * default `true`: gradient_method = GRAPE_GRAD_TAYLOR raises GRAPE_ERR_TAYLOR when a series has not reached
     * taylor_tolerance within taylor_max_order terms.  1 = `check_convergence = false`: the series is cut at
     * taylor_max_order terms and NO error is raised (terms below taylor_tolerance are still skipped: each of them changes
     * the result by less than the tolerance; the series kernels of N > 32 hold at most 64 terms -- a larger
     * taylor_max_order that is actually reached there is reported, not silently cut).  Ignored by GRAPE_GRAD_GRADGEN. */
    int32_t taylor_no_check;
} grape_problem;

/* Replaces GrapeWrk(...) data set-up: /root/reference/src/workspace.jl:147-362 */
int grape_create(grape_handle **out, const grape_problem *problem);
void grape_destroy(grape_handle *h);

/* Open quantum systems (entry points only: the ABI version stays 7).  The reference treats them as first class: the state is a
 * vectorised density matrix, the generator a Liouvillian super-operator (docs/src/background.md:46, :240-242).  Handing the
 * d^2 x d^2 Liouvillian to grape_create follows that recipe literally and ends at d = 22; a handle made by
 * grape_create_open propagates the d x d density matrices IN MATRIX FORM under a Lindblad generator, 2 <= d <= 64, with the
 * exact gradient (csrc/grape_lindblad.hip.h). */
typedef struct {
    int32_t J;              /* collapse operators, 0 <= J <= 8 (J = 0: unitary evolution of a density matrix)      */
    int32_t cops_per_traj;  /* 0: cops is [J][N*N], shared; 1: [K][J][N*N]                                         */
    const double *cops;     /* complex, column-major, rates folded in (A_j = sqrt(gamma_j) a_j); NULL iff J == 0   */
} grape_lindblad;
/* Meaning of grape_problem for such a handle: N = d; H0 [K][N*N], Hc, shape, tlist, weights, functional, K_total,
 * chi_min_norm, device as for grape_create; psi0 and target are [K][N*N] complex column-major MATRICES rho_k(0), sigma_k
 * (not required to be Hermitian or normalised: the evolution is linear).  On interval n
 *     H_kn   = H0_k + sum_l shape_ln eps_nl H_l                    (any complex matrices, as on the closed path)
 *     H_eff  = H_kn - (i/2) sum_j A_j^dagger A_j
 *     d rho / dt = L_kn(rho) = -i (H_eff rho - rho H_eff^dagger) + sum_j A_j rho A_j^dagger
 * tau_k = <<sigma_k|rho_k(T)>> = tr(sigma_k^dagger rho_k(T)); J_T_sm / ss / re, chi_k(T) = c_k sigma_k and the norm guard
 * (Frobenius norm) are the formulas above applied to that tau -- by construction what the vectorised problem gives (column
 * stacking, vec(A rho B) = (B^T (x) A) vec rho, generator i L in the role of H).  prop_tolerance: a series stops at
 * ||term||_F <= tol ||sum||_F (<= 0 selects 1e-17); the gradient is the exact derivative of the step (GRAPE_GRAD_GRADGEN).
 * Entry points that work on an open handle, with states [N*N] wherever this header says [N]: grape_eval, grape_forward,
 * grape_backward, grape_get_sums, grape_get_final_states, grape_backward_chi (chi [K][N*N]), grape_get_storage(which = 0)
 * ([K][N_T+1][N*N]), grape_get_tau_grads, grape_set_tlist, grape_eval_batch (one ordinary evaluation per set),
 * grape_get_timings ([1] forward launch, [2] backward launch, [5] both), grape_reset_timings, grape_get_work ([0] cells,
 * [2] / [3] flop of the matrix instructions the forward / backward launch executed, [7] series terms and [8] (sub-)steps of
 * the forward sweeps plus the backward chi chains; every other entry zero), grape_check, grape_last_error, grape_destroy.
 * target == NULL is legal exactly as for grape_create (forward + final states + grape_backward_chi).
 * GRAPE_ERR_INVALID with a message that names the reason, before the first HIP call: at create -- N > 64, J < 0, J > 8,
 * cops == NULL with J > 0, diss == NULL, gradient_method != GRAPE_GRAD_GRADGEN, prop_method != GRAPE_PROP_EXP, Dpen != NULL,
 * ndev > 1; later (the handle stays usable) -- grape_get_propagator, grape_get_storage(which = 1), grape_backward_xi,
 * grape_get_time_gradient (the time gradient of an open handle is grape_open_time_gradient, below), grape_forward_device,
 * grape_backward_device.  The state running cost of such a handle has entry points of its own: grape_open_set_running_cost and
 * grape_open_backward_xi, below. */
int grape_create_open(grape_handle **out, const grape_problem *problem, const grape_lindblad *diss);

/*
 * Replaces fg!(F, G, x): /root/reference/src/optimize.jl:105-111.
 *   G == NULL  -> evaluate_functional only (forward sweep, optimize.jl:696-768)
 *   G != NULL  -> evaluate_gradient!      (optimize.jl:824-1014); G has L*N_T doubles
 *   tau  (nullable) [K] complex  -> wrk.result.tau_vals      (optimize.jl:753)
 *   psiT (nullable) [K][N] complex -> fw_propagators[k].state (optimize.jl:187-189, 752)
 * Single-handle form: valid only when K == K_total.
 */
int grape_eval(grape_handle *h, const double *pulsevals, double *J, double *G, double *tau,
               double *psiT);

/*
 * Split-phase form for trajectory shards (one handle per GPU):
 *   1. grape_forward      : expm of every local cell + forward sweep; returns local tau[K]
 *   2. host all-reduces   : f = sum over ALL trajectories of w_k tau_k   (2 doubles)
 *   3. grape_backward     : chi from (f, local tau), backward sweep, per-cell derivatives and the
 *                           local sum over k; returns the PARTIAL gradient (L*N_T) and the local
 *                           partial sums needed for J ([2]=sum w|tau|^2, [3]=Re sum w tau, [4]=sum J_b)
 *   4. host all-reduces   : G (sum) -- the sum over k of optimize.jl:579
 * grape_eval() is exactly 1 + 3 with f computed locally.
 */
int grape_forward(grape_handle *h, const double *pulsevals, double *tau /* [K] complex */);
int grape_backward(grape_handle *h, const double f_total[2], double *G_partial);

/* The partial sums of this handle's trajectories after grape_forward -- what the host all-reduces in step 2 and what
 * every J_T and the state running cost need (J_parts[1], J_parts[3], optimize.jl:757-766):
 *   sums[0..1] = f = sum_k w_k tau_k, [2] = sum_k w_k |tau_k|^2, [3] = Re sum_k w_k tau_k,
 *   [4] = sum_k J_b,k (trapezoid sum of g_b, optimize.jl:727-750; multiply by lambda_b), [5..7] = 0. */
int grape_get_sums(grape_handle *h, double sums[8]);

/* Final states Psi_k(T) of the last forward sweep ([K][N] complex): `fw_propagators[k].state`, the argument of a
 * user-supplied J_T / chi (optimize.jl:752-760, 849-855). */
int grape_get_final_states(grape_handle *h, double *psiT);

/*
 * Backward half with HOST-SUPPLIED boundary states: chi[k] = chi_k(T) = -d J_T / d <Psi_k(T)| exactly as the user's
 * `chi(Psi, trajectories; tau)` returns them (optimize.jl:845-855; default constructor workspace.jl:306-308) --
 * [K][N] complex, NOT normalised.  The library adds the xi(T) term of the state running cost (:856-866), forms
 * rho_k = ||chi_k||, applies the chi_min_norm guard (:1021-1025), normalises (:867-868) and runs the backward sweep,
 * the per-cell derivatives and the sum over k.  Together with grape_forward + grape_get_final_states this keeps an
 * arbitrary J_T / chi pair on the caller's side: the three built-in functionals are only a fast path.
 * Returns the (partial, if sharded) gradient in G [L*N_T].
 */
int grape_backward_chi(grape_handle *h, const double *chi, double *G);

/* ABI v5.  An ARBITRARY state running cost g_b (optimize.jl:727-750, 856-866, 897-908: the reference calls the user's
 * g_b(state, trajectory, tlist, n) and xi(state, trajectory, tlist, n) = -d g_b / d<Psi| inside its loops; callbacks cannot
 * cross a C ABI, so the data does): after grape_forward the caller reads the stored forward states
 * (grape_get_storage(0): Psi_k(t_n), [K][N_T+1][N]), evaluates g_b and xi on them, and hands back
 *   xi       : [K][N_T+1][N] complex, xi_k(t_n) (entry n = 0 is not used, as in the reference),
 *   lambda_b : the weight of J_b in J.
 * The library adds lambda_b dt/2 xi_k(T) to chi_k(T) (optimize.jl:856-866) and lambda_b Dt_n / rho_k xi_k(t_n) behind
 * every backward step (:897-908, trapezoid weights of :727-750) and returns the gradient of J_T + lambda_b J_b.  chi:
 * [K][N] boundary states of a user-defined J_T as in grape_backward_chi, or NULL for the handle's built-in functional
 * (then f_total = all-reduced sum_k w_k tau_k as in grape_backward).  J_b itself is the caller's trapezoid sum of g_b.
 * (The built-in family g_b = <Psi|D|Psi> of grape_problem.Dpen stays the device-side fast path.) */
int grape_backward_xi(grape_handle *h, const double f_total[2], const double *chi, const double *xi, double lambda_b,
                      double *G);

/* Device-resident variants used by the bench / RCCL path: same semantics, every pointer is a
 * device pointer on the handle's device; work is enqueued on `stream` (a hipStream_t passed as
 * void*) without host synchronisation (single-device handles only).
 *   d_out layout of grape_forward_device (2K + 8 doubles): [0..2K) tau, then the shard sums
 *        [2K] Re f, [2K+1] Im f (f = sum_k w_k tau_k), [2K+2] sum_k w_k |tau_k|^2,
 *        [2K+3] Re sum_k w_k tau_k, [2K+4] sum_k J_b,k (state running cost), [2K+5..2K+7] 0
 *   d_f   : 2 doubles, the all-reduced f;  d_G: L*N_T doubles (partial gradient, overwritten) */
int grape_forward_device(grape_handle *h, const double *d_pulsevals, double *d_out, void *stream);
int grape_backward_device(grape_handle *h, const double *d_f, double *d_G, void *stream);

/* Concurrent sweeps.  With one workgroup per trajectory a sweep occupies K of the 256 CUs, and the backward
 * recursion chi_{n-1} = U_n^dagger chi_n (optimize.jl:881) is linear in chi; so, unless the state running cost adds its
 * inhomogeneity, grape_forward[_device] also runs the backward sweep, from the unit targets, in the same launch, and
 * grape_backward[_device] only applies the boundary coefficient of chi_k(T) = c_k target_k (docs/src/tutorial.md:402)
 * to the overlaps.  Results are identical to rounding.  on = 0 restores the sequential order (a caller that only wants
 * tau from the split-phase API should do that; grape_eval with G == NULL never runs the backward sweep).  Returns 1 if
 * the concurrent path is active for this handle afterwards, 0 if not.  Default: on (env GRAPE_FUSED_SWEEPS=0: off). */
int grape_set_fused_sweeps(grape_handle *h, int on);

/* Synchronise `stream` and translate the device-side error flags of the evaluation in flight
 * (singular Pade denominator, chi norm guard, series non-convergence) into a grape_status. */
int grape_check(grape_handle *h, void *stream);

/* U_kn = exp(-i H_kn dt_n) of the last evaluation as an N x N column-major complex matrix
 * (parity check of the ExpProp step, optimize.jl:732). */
int grape_get_propagator(grape_handle *h, int k, int n, double *out);

/* Optional outputs of the last evaluation (debug / parity): tau_grads[k][l][n] complex
 * (workspace.jl:236-237, value of optimize.jl:894), forward storage [k][n][N] complex
 * (workspace.jl:215; n = 0..N_T) and the backward states chi_k(t_n) [k][n][N]. */
int grape_get_tau_grads(grape_handle *h, double *out /* K*L*N_T complex */);
int grape_get_storage(grape_handle *h, int which /*0 fw, 1 bw*/, double *out /* K*(N_T+1)*N complex */);

/* Per-phase device time in milliseconds, measured with HIP events recorded on the stream the
 * kernels were launched on, AVERAGED over the evaluations since the last grape_reset_timings
 * (at most the 64 most recent): [0] expm kernel, [1] forward sweep, [2] backward sweep,
 * [3] cell derivatives, [4] reduction, [5] whole grape_eval; handles with several devices (ndev > 1) also [6] the host
 * wall time of the enqueue halves per evaluation (every shard is enqueued from its own host thread) and [7] the latency of
 * the RCCL all-reduce of the gradient across the shards (HIP events on the first shard's stream; -1 when the reductions
 * are host-staged: repeated device ordinals, GRAPE_MULTI_RCCL=0, RCCL not loadable).  Synchronises the device.
 * Returns the number of entries written. */
int grape_get_timings(grape_handle *h, double *ms, int n);
int grape_reset_timings(grape_handle *h);
/* Algorithmic work of the last evaluation: [0] cells, [1] sum of squarings s over cells,
 * [2] flop of the expm kernel (SURVEY 8d F_exp), [3] flop of the derivative kernel, [4] derivative series orders,
 * [5] cells solved by the pivoted fallback, [6] propagators exponentiated, [7] terms and [8] (sub-)steps of the
 * matrix-free propagator, [9] flop of the matrix instructions EXECUTED by the inverse-free exponential of Hermitian
 * generators (grape_t18.hip.h), [10] its squarings, [11] its cells, [12] 1 when prop_method = GRAPE_PROP_EXP was asked for
 * but the propagators (KC N_T NP^2 16 bytes) do not fit the device and the handle evaluates matrix-free instead of
 * failing in hipMalloc (same results to rounding; shards of a composite handle: the number of shards in that mode),
 * [13] the cells of [11] that took the four-product degree-16 route (Hermitian generators, 16 < N <= 64, spectral bound
 * within its range), [14] 1 if the four-product route of this handle is the hand-allocated assembly kernel (csrc/asm/gen_t16.py:
 * Hermitian generators, 49 <= N <= 64, control operators shared by the trajectories; GRAPE_EXPM_ASM=0: the C++ kernel), 2 if
 * the exponential of this handle is the assembly cell for GENERAL matrices (csrc/asm/gen_t18g.py: non-Hermitian drift or
 * controls, same sizes; GRAPE_EXPM_ASM18G=0: the C++ kernel), 3 if it is the four-product assembly cell for control operators
 * per trajectory (csrc/asm/gen_t16p.py: Hermitian generators, up to four controls; GRAPE_EXPM_ASM16P=0), 4 the same for general matrices (gen_t18gp.py: one or two controls),
 * [15] the derivative kernel of the ExpProp route: 0 a compiled kernel, 1 deriv3_asm (49 <= N <= 64, Hermitian, L <= 2),
 * 2 deriv3s_asm (3 <= L <= 8, controls streamed through the LDS), 3 deriv3g_asm (general drift / controls), 4 deriv4_asm
 * (64 < N <= 256), [16] 1 if the products of the blocked polynomial route are the assembly kernel lg_gemm_asm,
 * [17] the steps of the two sweeps that the walks of the exponential kernel carried in the last evaluation (the sweep
 * launch did the remaining 2 K N_T - [17]), [18] the block length of the scanned sweeps of N <= 64 (round 6: the time axis is
 * cut into blocks whose propagators are formed first; by default from 64 time steps on, with at most 96 / 64 / 48 / 24
 * generator classes at NP = 16 / 32 / 48 / 64; 0: sequential sweeps; GRAPE_SCAN16=0 / 1 forces)
 * [19] the cells of the last evaluation whose spectrum was certified before the launch of the four-product assembly kernel:
 * tr H^8 and tr H^6 of H = H0_k + sum_l e_l C_l are polynomials in the pulse values whose coefficients grape_create tabulates
 * per generator class (Hermitian generators, 1 <= L <= 4, assembly route); the plan of an evaluation tests
 * (p8 + 2^-30 S8) dt^8 (1 + 1e-6) <= (1.36 * 2^s)^8 and p6 >= 0 on them and a cell that passes skips the spectral bound it
 * would otherwise compute from its own products -- the same inequality with a narrower margin, so the results are the same
 * bits.  0 on handles without tables, with GRAPE_EXPM_CERT=0, and when the plan skipped the route,
 * [20] the cells (counted per trajectory) of the last evaluation that qualified for the shortest economized derivative series
 * (degree 15, spectral radius <= 1.11): verdict 0, no planned squarings, and certified by the plan from tr H^4, tr H^8 and
 * tr H^12 (tables of grape_create: Hermitian generators, 1 <= L <= 2, assembly route; GRAPE_DERIV_SEG=0: no tables).  A batch of
 * 16 cells still runs the largest degree of its cells (grape_get_work[4] says what ran).  0 on handles without these tables,
 * [21] the cells of the last evaluation whose second product ran as a Hermitian square (csrc/asm/gen_t16q.py, coefficient set
 * T16Q_* with c2 = 0: 625 instead of 697 matrix instructions per wave): cells with no planned squarings that the plan certified
 * both for the range of the four products (the inequality of [19] at s = 0) and for the segment 1.11 (the three moments of
 * [20]); Hermitian generators, shared controls, 1 <= L <= 2, assembly route.  GRAPE_EXPM_T16Q=0: never, 1: every such handle,
 * unset: handles whose launch gives every workgroup a walk of at least 8 cells.  Independent of GRAPE_EXPM_CERT,
 * GRAPE_DERIV_SEG and GRAPE_DERIV_ECON.  0 on other handles and when the plan skipped the route,
 * [22] 1 when the kernel that ran the cells of [21] was expm_t16r_asm (csrc/asm/gen_t16r.py): the arithmetic of expm_t16q_asm
 * operation for operation -- the same bits -- with the tile exchanges of the two Hermitian squares sent under the last matrix
 * instructions of the square, and 624 matrix instructions per marked cell and wave ([9] books them).  GRAPE_EXPM_T16R=0: never,
 * 1: wherever [21] counts cells of the assembly route, unset: where that route is on by its own rule and not by
 * GRAPE_EXPM_T16Q=1.  [14] stays 1
 * (entries beyond n are not written). */
int grape_get_work(grape_handle *h, double *out, int n);

/* The trace tables behind grape_get_work[19] (diagnostics, tests).  dims [3] = KC, n8, n6: generator classes, coefficients of
 * tr H^8 and of tr H^6 (45 and 28 at L = 2; both 0: this handle has no tables).  coef (NULL: not wanted) [KC][n8 + n6]: t8 | t6
 * of every class; exps (NULL: not wanted) [n8 + n6]: the exponents of e_1 .. e_L of the monomial a coefficient multiplies, four
 * bits each, e_1 lowest (e_l = pulse value times shape).  GRAPE_ERR_INVALID: h or dims NULL, an open handle, several devices. */
int grape_get_cert_table(grape_handle *h, int *dims, double *coef, int *exps);

/* The tables behind grape_get_work[20] (diagnostics, tests), as the plan of an evaluation reads them.  dims [4] = KC, n4, n8, n12:
 * generator classes, coefficients of tr H^4, tr H^8 and tr H^12 (15, 45 and 91 at L = 2; all 0: this handle has no segment tables).
 * coef (NULL: not wanted) [KC][n4 + n8 + n12]: t4 | t8 | t12 of every class -- t8 is the certificate's table above when the handle
 * has it, the segment tables' own copy with GRAPE_EXPM_CERT=0; exps (NULL: not wanted) [n4 + n8 + n12]: exponents as above.
 * GRAPE_ERR_INVALID: h or dims NULL, an open handle, several devices. */
int grape_get_seg_table(grape_handle *h, int *dims, double *coef, int *exps);

/* ABI v7.  Derivative of J with respect to the time steps dt_n = tlist[n+1] - tlist[n] (0-based n < N_T), for the duration
 * loop around GRAPE (INTEGRATION.md "Optimising the duration").  For piecewise-constant generators dU_n/d(dt_n) = -i H_n U_n:
 *   dJdt[n] = -2 Re sum_k f_k <chi_k(t_{n+1})| (-i H_kn) |Psi_k(t_{n+1})>  (+ lambda_b / 2 sum_k (g_b,k(t_n) + g_b,k(t_{n+1})))
 * from the states the last evaluation stored (f_k: the factor of tau_grads), the same reduction as the gradient
 * (optimize.jl:574-584).  Call it after anything that ran the backward half: grape_eval with G != NULL, grape_backward,
 * grape_backward_chi, grape_backward_xi, grape_backward_device (after a device-pointer call on a foreign stream it waits
 * for the device, as the other getters).  It launches its kernel on demand: evaluations that never call it are unchanged.
 * GRAPE_ERR_INVALID (handle stays usable): no evaluation yet, the last one had no gradient or failed, between grape_forward
 * and the backward half, or grape_set_tlist since.
 *   - single handle (K == K_total): the full derivative; split-phase shard (K < K_total): the partial sum over its own
 *     trajectories, which the caller all-reduces like G; several devices behind one handle: the sum over its shards.
 *   - the built-in running cost (grape_problem.Dpen, lambda_b) includes the explicit derivative of its trapezoid weights
 *     (optimize.jl:727-750).  After grape_backward_xi (the caller's g_b) the result is the propagation part ONLY: the
 *     caller adds lambda_b / 2 sum_k (g_b,k(t_n) + g_b,k(t_{n+1})) for interval n, because only the caller has g_b.
 *   - the derivative is taken at fixed per-interval pulse and shape values.  A shape S(t) (or pulse) sampled at the
 *     interval midpoints moves when dt_n changes; that chain rule is the caller's.
 *   - grid-point form: with t_0 fixed, dJ/dt_j = dJdt[j-1] - dJdt[j] (1 <= j < N_T), dJ/dt_{N_T} = dJdt[N_T-1].
 *     Scaling a grid of duration T: dJ/dT = sum_n (dt_n / T) dJdt[n]. */
int grape_get_time_gradient(grape_handle *h, double *dJdt /* [N_T] */);

/* The same derivative for an open-system handle (grape_create_open; an entry point only, the ABI version stays 7;
 * csrc/grape_lindblad_tg.hip.h).  exp(L_n dt_n) commutes with L_n, so
 *   dJdt[n] = dJ/d(dt_n) = -2 Re sum_k <<chi_k(t_{n+1}) | L_kn rho_k(t_{n+1})>> = -2 Re sum_k <<L_kn^dagger chi_k(t_{n+1}) | rho_k(t_{n+1})>>
 * with the stored forward states and the chi chain stepped back from chi_k(T): exact to rounding whatever the number of
 * sub-steps, and at the cost of about one forward launch.  Under a Lindblad generator every extra moment costs fidelity, so
 * the optimal duration is an interior optimum and this derivative locates it.
 * Valid after a successful backward half on the current grid: grape_eval with G != NULL, grape_backward (chi_k(T) = c_k
 * sigma_k with the f that call received, tau_k under J_T_ss), or grape_backward_chi (the caller's chi_k(T), which the handle
 * still holds on the device).  A split-phase shard (K < K_total) returns the partial sum over its own trajectories, to be
 * all-reduced like G.  Fixed per-interval pulse and shape values, grid-point form and dJ/dT as for grape_get_time_gradient.
 * It launches its kernel on demand and owns its buffers (allocated by the first call, freed by grape_destroy): evaluations
 * that never call it are unchanged; after it grape_get_tau_grads, grape_get_work, grape_get_timings and grape_get_storage
 * return what they returned before and a grape_eval is bit for bit what it was.  Two calls give the same bits.
 * GRAPE_ERR_INVALID with a message that names the reason (the handle stays usable): h == NULL (message: grape_last_error(NULL)),
 * dJdt == NULL, a closed handle (use grape_get_time_gradient), no evaluation yet, the last evaluation had no gradient or
 * failed, between grape_forward and the backward half, grape_set_tlist since, grape_eval_batch since.  GRAPE_ERR_TAYLOR: a
 * series of the chi chain did not converge (cannot happen after a successful backward half, but is never silent). */
int grape_open_time_gradient(grape_handle *h, double *dJdt /* [N_T] */);

/* ABI v7.  Replaces the time grid of an existing handle (N_T unchanged): tlist [N_T+1], finite and strictly increasing as in
 * grape_create, else GRAPE_ERR_INVALID and the handle is unchanged.  Waits for work in flight, recomputes the time steps and
 * the trapezoid weights on every shard and device, drops the captured graph of the single-wait evaluation and resets the
 * launch plan of the blocked path: the next evaluation gives what a handle created with this grid gives.  Results of the
 * previous grid (stored states, the time gradient) are no longer available; the next call must be a forward evaluation. */
int grape_set_tlist(grape_handle *h, const double *tlist /* [N_T+1] */);

/* Many pulse vectors at once (entry points only: the ABI version stays 7).  P pulse vectors through the problem of ONE
 * handle -- the starts of a multi-start optimisation, a population of optimisers, the trial points of a line search, a scan
 * over amplitudes: the same fg!(F, G, x) (optimize.jl:105-111) at P different x.  Element p of every output is what
 * grape_eval(h, pulsevals + p*L*N_T, &J[p], G + p*L*N_T, tau + 2*p*K, NULL) returns:
 *   pulsevals [P][L*N_T] control-major per set (a column-major Julia matrix L*N_T x P);  J [P];
 *   G NULL or [P][L*N_T] (NULL: functional only, no backward half);  tau NULL or [P][K] complex.
 * Valid only when K == K_total (as grape_eval).  One in-flight call per handle, host pointers are not retained.
 *   - Routes.  Inside the envelope of the batched kernels -- one device, N <= 16, GRAPE_PROP_EXP with propagators that fit,
 *     GRAPE_GRAD_GRADGEN, no built-in running cost (Dpen); Hermitian and general generators, shape, non-uniform grids,
 *     hc_per_traj 0 and 1, the three functionals, weights, L <= 8 -- the pulse set is one more grid axis of the kernels
 *     (csrc/grape_batch.hip.h): all sets of a launch group run side by side, a set's result does not depend on its
 *     neighbours or on the grouping (bit for bit), and agrees with grape_eval to rounding.  Everything else (N > 16,
 *     GRAPE_GRAD_TAYLOR, GRAPE_PROP_SERIES, Dpen, ndev > 1, the matrix-free fallback of grape_get_work[12]) takes one ordinary
 *     evaluation per set inside the library: bit for bit the results of P grape_eval calls.  Inside the envelope a route
 *     rule chooses (a single set, or an ensemble that fills the chip by itself, is better off on the ordinary path);
 *     environment GRAPE_BATCH=0 / 1, read by grape_create, forces the loop / the batched kernels (outside the envelope
 *     always the loop).  The batched route cuts P into launch groups that fit a memory budget (GRAPE_BATCH_SETS=<n>,
 *     read by grape_create, sets the group size); its storage is allocated by the first batch call, grows on demand and is
 *     freed by grape_destroy.  It reads the current time grid (grape_set_tlist) and always runs the concurrent sweeps
 *     (grape_set_fused_sweeps does not enter: the results are identical to rounding).
 *   - Errors.  h == NULL, P <= 0, pulsevals == NULL, J == NULL, a split-phase shard (K < K_total), a handle without targets:
 *     GRAPE_ERR_INVALID, handle unchanged and usable.  If the evaluation of a set raises a device-side status
 *     (GRAPE_ERR_CHI_NORM, GRAPE_ERR_TAYLOR, GRAPE_ERR_SINGULAR) the call returns the status of the lowest such p,
 *     grape_last_error names that p ("pulse set p: ..."), the outputs are unspecified and the handle stays usable.
 *   - State afterwards.  The "last evaluation" that grape_get_storage, _tau_grads, _propagator, _final_states and _sums refer
 *     to is NOT defined after a batch call; grape_get_time_gradient returns GRAPE_ERR_INVALID until the next ordinary
 *     evaluation with a gradient.  An ordinary grape_eval after a batch call gives exactly what it gave before it: the
 *     batched route owns its buffers and touches neither the captured graph nor the scan set-up nor the launch plans. */
int grape_eval_batch(grape_handle *h, int P, const double *pulsevals, double *J, double *G, double *tau);

/* What the last grape_eval_batch of this handle did: [0] 1 = batched kernels, 0 = one ordinary evaluation per set;
 * [1] sets per launch group;  [2] number of groups;  [3] bytes of batch storage the handle holds on the device.
 * Returns the number of entries written (at most n). */
int grape_get_batch_info(grape_handle *h, double *out, int n);

/* Exact Hessian-vector products of J (entry points only: the ABI version stays 7).  What a Newton-CG or trust-region solver
 * needs near convergence, where the gradient alone stalls (the reference names "a true Hessian of the optimization
 * functional" as future work, paper/paper.md:42; Goodwin & Kuprov 2016):
 *   HV[j] = (d^2 J / d eps^2) V[j],  j < nv,  at the pulses of the last evaluation;  V, HV: [nv][L*N_T], control-major.
 * J is the handle's built-in functional (J_T_sm / ss / re with weights, K == K_total).  The product is the derivative of
 * the gradient along V[j], taken term by term through the series of every step (csrc/grape_hvp.hip.h): exact
 * to rounding like the gradient itself, not a difference of two gradients.
 *   - Valid after any successful evaluation that ran the forward half on the current time grid: grape_eval with or without
 *     G, grape_forward with or without its backward half.  It reads only the stored forward states, tau, f and the device
 *     copy of the pulses and recomputes the backward chain itself: the result does not depend on the backward storage, on
 *     the concurrent sweeps, or on which exponential / derivative kernel ran (GRAPE_PROP_EXP, GRAPE_PROP_SERIES and the
 *     matrix-free fallback alike).  General generators, hc_per_traj, shape and non-uniform grids as grape_eval.
 *   - The directions are a grid axis of the kernels; a direction's result does not depend on nv or on the launch groups
 *     (bit for bit), and results are bitwise repeatable.  The storage is allocated by the first call, grows with nv in
 *     launch groups under a memory budget (GRAPE_HVP_DIRS=<n>, read by grape_create, sets the group size) and is freed
 *     by grape_destroy.  The call touches neither the captured graph nor the scan set-up nor the launch plans: a
 *     grape_eval after it returns bit for bit what it returned before, and grape_get_time_gradient still works.
 *   - Series: m = ceil(beta_n dt_n / theta) sub-steps from the create-time norm estimates; a series stops when every chain
 *     has ||term|| <= prop_tolerance ||sum|| (default 1e-17), after at most 200 terms -- beyond that GRAPE_ERR_TAYLOR, the
 *     handle stays usable.
 *   - GRAPE_ERR_INVALID with a message that names the reason, the handle stays usable: h == NULL, nv <= 0, V == NULL,
 *     HV == NULL; N > 64; ndev > 1; a split-phase shard (K < K_total); an open-system handle (grape_open_hvp is the call
 *     for one); a handle without targets; the
 *     built-in running cost (Dpen, lambda_b != 0); no valid forward state (no evaluation yet, the last one failed,
 *     grape_set_tlist came since, or the last call was grape_eval_batch).  A caller-supplied chi (grape_backward_chi)
 *     is out of scope: it would need the caller's chi'(T).  The full Hessian is nv = L*N_T unit directions. */
int grape_hvp(grape_handle *h, int nv, const double *V, double *HV);

/* What the last grape_hvp of this handle did: [0] series terms and [1] (sub-)steps summed over the workgroups of both
 * sweeps (every (trajectory, direction) pair walks N_T intervals forwards and N_T backwards: 2 K nv N_T steps when no
 * interval is cut);  [2] directions per launch group;  [3] bytes of HVP storage the handle holds;  [4] milliseconds of the
 * last call (host wall time, copies included);  diagnostics behind them: [5] the series terms of the tangent forward sweeps,
 * [6] of the backward sweeps ([0] = [5] + [6]; tools/hvp_ab.py counts the executed matrix instructions from them).
 * Returns the number of entries written (at most n). */
int grape_get_hvp_info(grape_handle *h, double *out, int n);

/* The exact Hessian of J as a matrix, in one call (entry points only: the ABI version stays 7; csrc/grape_hessian.hip.h,
 * DESIGN.md 25).  What Newton-Raphson / RFO GRAPE with a regularised Hessian (Goodwin & Kuprov 2016), scipy's trust-exact
 * and any look at the curvature of a converged pulse need (saddle points, conditioning, error bars):
 *   H[p][q] = d^2 J / d eps_p d eps_q,  p, q < P = L*N_T, indexed as G (p = l*N_T + n), at the pulses of the last evaluation;
 *   H: [P][P] doubles, the full symmetric matrix (both triangles, bitwise symmetric).
 * J is the handle's built-in functional (J_T_sm / ss / re with weights, K == K_total).  Exact to rounding like grape_hvp:
 * H[:, q] is what grape_hvp returns for the unit direction e_q -- but a unit direction spends two full sweeps on a tangent
 * that is zero before its interval and merely propagated after it.  Here the first derivatives of every interval are
 * formed once (forward from the stored Psi_k(t_n), backward from the bare targets), carried forwards sixteen columns to a
 * matrix tile from the interval where they are born, and overlapped at every grid point; the diagonal blocks come from
 * the second-order series of the backward chain, the coupling of the trajectories through f from a closed boundary term.
 *   - Valid when grape_hvp is valid: after any successful evaluation that ran the forward half on the current time grid.
 *     It reads only the stored forward states, tau, f, the device copy of the pulses and the static data of the handle
 *     (balanced frame): the result does not depend on which exponential / derivative route ran.
 *   - The storage is the handle's, allocated by the first call and freed by grape_destroy: 2 K N_T L NP 16 bytes of first
 *     derivatives, two P x P matrices, and 8 P^2 bytes plus step matrices per trajectory of a pass.  The trajectories are
 *     taken in passes under the memory budget of grape_hvp (8 GB, half of the free memory; GRAPE_HESS_TRAJ=<n>, read by
 *     grape_create, sets the pass size); the passes are summed one trajectory after the other in ascending k, so the
 *     result does not depend on the budget or on the passes, bit for bit.  Two calls give the same bits.
 *   - The call runs on the handle's stream outside the captured graph and touches neither the scan set-up, the launch
 *     plans nor the storage of grape_hvp and its halves: a grape_eval after it returns bit for bit what it returned
 *     before; grape_get_time_gradient, grape_hvp, grape_expect and a pending grape_hvp_backward still answer.
 *   - Series as grape_hvp: m = ceil(beta_n dt_n / theta) sub-steps, a series stops when every column has
 *     ||term|| <= prop_tolerance ||sum||, after at most 200 terms -- beyond that GRAPE_ERR_TAYLOR, the handle stays usable.
 *   - GRAPE_ERR_INVALID with a message that begins "grape_hessian:" and names the reason, before anything touches the
 *     device, the handle stays usable: h == NULL (message through grape_last_error(NULL)), H == NULL; an open-system
 *     handle; ndev > 1; N > 64; L > 4 (grape_hvp with unit directions is the route); L*N_T > 8192; a split-phase shard
 *     (K < K_total); a handle without targets; the built-in running cost (Dpen, lambda_b != 0) or a last backward half that
 *     took a caller's xi; no valid forward state (no evaluation yet, the last one failed, grape_set_tlist came since, or
 *     the last call was grape_eval_batch).  A caller's chi and mixed derivatives with respect to the time steps are out of
 *     scope.
 *   - GRAPE_ERR_HIP with the sizes in the message when the storage cannot be allocated (even for one trajectory per pass);
 *     nothing stays allocated then. */
int grape_hessian(grape_handle *h, double *H);

/* What the last grape_hessian of this handle did: [0] series terms and [1] (sub-)steps summed over all workgroups of the
 * call;  [2] trajectories per pass;  [3] bytes of Hessian storage the handle holds;  [4] milliseconds of the last call (host
 * wall time, copies included);  [5] / [6] / [7] the series terms of the forward seeds / the backward seeds / the fan
 * ([0] = [5] + [6] + [7]).  Returns the number of entries written (at most n). */
int grape_get_hessian_info(grape_handle *h, double *out, int n);

/* grape_hessian for a handle made by grape_create_open (entry points only: the ABI version stays 7, grape_problem and
 * grape_lindblad are untouched; csrc/grape_lindblad_hessian.hip.h):
 *   H[p][q] = d^2 J / d eps_p d eps_q,  p, q < P = L*N_T, indexed as G (p = l*N_T + n), at the pulses of the last evaluation;
 *   H: [P][P] doubles, the full symmetric matrix (both triangles, bitwise symmetric).
 * J is the handle's built-in functional (J_T_sm / ss / re with weights, K == K_total).  Column q is what grape_open_hvp returns
 * for the unit direction e_q, to rounding -- without its two full sweeps and its four-chain backward recursion per control
 * and direction: the first derivatives of every interval are formed once (forward from the stored rho_k(t_n), backward
 * from the bare targets sigma_k), every forward derivative is carried on from the interval where it is born and overlapped
 * at every later grid point, the diagonal blocks come from the second-order chain of the backward seeds, the coupling of the
 * trajectories through f from a closed boundary term.  Hermitian and general drift, per-trajectory control and collapse
 * operators, shape functions, non-uniform grids and weights are all inside; d <= 64, J <= 8 as the handle itself.
 *   - Valid exactly when grape_open_hvp is valid: after a successful forward half on the current time grid.  It reads only
 *     the stored rho_k(t_n), tau, f, the device copy of the pulses and the static data of the handle.
 *   - The storage is the handle's, allocated by the first call and freed by grape_destroy: 2 K N_T L matrices (2 NP^2
 *     doubles each) of first derivatives, K (N_T+1) of the bare target chain, two P x P matrices, seed workspaces (up to
 *     about 512 (14 + 4J) matrices), and 8 P^2 bytes plus fan workspaces per
 *     trajectory of a pass.  The trajectories are taken in passes under the memory budget of grape_open_hvp (8 GB, half of
 *     the free memory; GRAPE_OPEN_HESS_TRAJ=<n>, read by grape_create_open, sets the pass size) and summed one after the
 *     other in ascending k: the result does not depend on the passes, bit for bit.  GRAPE_OPEN_HESS_COLS=<n> (1 ... 16, read
 *     by grape_create_open) sets how many columns one workgroup of the fan carries; a column's bits do not depend on it.
 *     Two calls give the same bits.
 *   - The call runs on the handle's stream and leaves alone the storage of grape_open_hvp and its halves, the validity
 *     words, the statistics and the timings of the evaluation: grape_eval, grape_get_tau_grads, grape_open_time_gradient,
 *     grape_open_hvp and grape_expect return the bits they returned before, a pending grape_open_hvp_backward still answers.
 *   - Series as grape_open_hvp: m = ceil(beta_n dt_n / theta) sub-steps, a series stops when every chain has
 *     ||term||_F <= prop_tolerance ||sum||_F, after at most 200 terms -- beyond that GRAPE_ERR_TAYLOR, the handle stays usable.
 *   - GRAPE_ERR_INVALID with a message that begins "grape_open_hessian:" and names the reason, before anything touches the
 *     device, the handle stays usable: h == NULL (message through grape_last_error(NULL)), H == NULL; a closed handle
 *     (grape_hessian is the call); L > 4 (grape_open_hvp with unit directions is the route); L*N_T > 8192; a split-phase
 *     shard (K < K_total); a handle without targets; a running cost set by grape_open_set_running_cost; no valid forward
 *     state, with the distinctions of grape_open_hvp (no evaluation yet, the last forward sweep failed, grape_set_tlist or
 *     grape_open_set_running_cost came since, the last call was grape_eval_batch).
 *   - GRAPE_ERR_HIP with the sizes in the message when the storage cannot be allocated (even for one trajectory per pass);
 *     nothing stays allocated then. */
int grape_open_hessian(grape_handle *h, double *H);

/* What the last grape_open_hessian of this handle did: [0] series terms and [1] (sub-)steps summed over all workgroups of
 * the call;  [2] trajectories per pass;  [3] bytes of Hessian storage the handle holds;  [4] milliseconds of the last call
 * (host wall time, copies included);  [5] / [6] / [7] the series terms and [8] / [9] / [10] the (sub-)steps of the forward
 * seeds / the backward seeds / the fan;  [11] columns per workgroup of the fan.  Returns the number of entries written (at
 * most n), GRAPE_ERR_INVALID on a closed handle. */
int grape_get_open_hessian_info(grape_handle *h, double *out, int n);

/* grape_hvp in two halves, cut at its one cross-trajectory dependency (entry points only, the ABI version stays 7;
 * csrc/grape_hvp_split.hip.h).  What grape_hvp refuses -- a trajectory shard (K < K_total) and a caller's
 * functional, handles without targets included -- goes through these, as the gradient goes through grape_forward +
 * grape_backward / grape_backward_chi.  grape_hvp itself and its refusals are unchanged.
 *
 * grape_hvp_forward: the tangent forward sweep of nv directions V [nv][L*N_T] at the pulses of the last evaluation.  It
 * leaves Psi'_k(t_n) of ALL nv directions on the device and returns, each where the pointer is not NULL,
 *     dtau  [nv][K] complex     tau'_k = <tgt_k | Psi'_k(T)>
 *     dsums [nv][2]             sum over THIS handle's k of w_k tau'_k -- what the host all-reduces between the halves
 *     dpsiT [nv][K][N] complex  Psi'_k(T) in the caller's frame (what a caller's chi' is formed from)
 * It needs what grape_hvp needs: a successful evaluation that ran the forward half on the current time grid.  On a handle
 * without targets dtau and dsums come back NaN, as tau does.
 *
 * grape_hvp_backward: the built-in functional.  f_total is the all-reduced sum_k w_k tau_k (as for grape_backward),
 * df_total [nv][2] the all-reduced dsums.  It uses K_total and the handle's weights.  On an unsharded handle
 * grape_hvp_forward + grape_hvp_backward(grape_get_sums()[0:2], dsums) gives the bits of grape_hvp.
 *
 * grape_hvp_backward_chi: a caller's functional.  chi [K][N] complex = chi_k(T) as for grape_backward_chi, dchi [nv][K][N]
 * its derivative along V[j] (both in the caller's frame; not normalised, no chi_min_norm guard: everything is linear in
 * chi).  It reads neither targets, weights, tau, f nor the functional.
 *
 *   - HV [nv][L*N_T] is the sum over this handle's trajectories: the full product when K == K_total, otherwise the partial
 *     sum the caller all-reduces like G.
 *   - A backward half needs a successful grape_hvp_forward with the same nv since the last of: any forward evaluation,
 *     grape_set_tlist, grape_eval_batch, grape_hvp (it shares the tangent storage and overwrites it).  Otherwise
 *     GRAPE_ERR_INVALID with a message that names which of these came between; the handle stays usable.  Any number of
 *     backward halves, of either kind, may follow one forward half.
 *   - All nv directions stay resident between the halves: an nv beyond the storage budget of grape_hvp (8 GB, half of the
 *     free memory) or beyond GRAPE_HVP_DIRS is GRAPE_ERR_INVALID, the message names the largest nv that fits; the caller
 *     loops.  What only the split calls need is allocated by the first of them, in a store of its own.
 *   - A direction's result does not depend on nv or on its position, and two calls give the same bits.  Nothing an
 *     evaluation, grape_get_time_gradient or grape_hvp reads is touched.
 *   - grape_get_hvp_info: after a forward half [5] = [0] = its series terms and [6] = 0; after a backward half [6] and
 *     [0] = [5] + [6]; [1] the (sub-)steps of both halves; [4] the milliseconds of the last call.
 *   - A series that does not converge within 200 terms: GRAPE_ERR_TAYLOR, as in grape_hvp.
 *   - GRAPE_ERR_INVALID with a message that names the reason, before the first HIP call: h == NULL (message:
 *     grape_last_error(NULL)); a NULL V / HV / chi / dchi / f_total / df_total; nv <= 0; an open-system handle; N > 64;
 *     ndev > 1; the built-in running cost (Dpen, lambda_b != 0) or a handle whose last backward half took a caller's xi;
 *     grape_hvp_backward on a handle without targets (grape_hvp_backward_chi is the route). */
int grape_hvp_forward(grape_handle *h, int nv, const double *V, double *dtau, double *dsums, double *dpsiT);
int grape_hvp_backward(grape_handle *h, int nv, const double f_total[2], const double *df_total, double *HV);
int grape_hvp_backward_chi(grape_handle *h, int nv, const double *chi, const double *dchi, double *HV);

/* Exact Hessian-vector products on an open-system handle (grape_create_open; entry points only, the ABI version stays 7;
 * csrc/grape_lindblad_hvp.hip.h):
 *   HV[j] = (d^2 J / d eps^2) V[j],  j < nv,  at the pulses of the last evaluation;  V, HV: [nv][L*N_T], control-major.
 * J is the handle's built-in functional (J_T_sm / ss / re with weights, K == K_total).  With B = sum_l v_nl s_ln D_l the
 * directional derivative of the generator of interval n, a tangent forward sweep carries rho'_k next to the STORED rho_k(t_n)
 * (u'_{a+1} = h / (a+1) (L u'_a + B u_a)), chi'_k(T) = c'_k sigma_k (sm: w_k f' / K^2, ss: w_k tau'_k / K, re: 0), and a
 * backward sweep carries chi, chi', P_l, P'_l under L^dagger:
 *   (H v)_nl = -2 Re sum_k [ <<P'_l | rho_k(t_n)>> + <<P_l | rho'_k(t_n)>> ]
 * exact to rounding like the gradient, term by term through the series of every (sub-)step; not a difference of gradients.
 *   - Valid after any successful forward half on the current grid: grape_eval with or without G, grape_forward with or
 *     without its backward half.  It reads only the stored forward states, tau, f and the device copy of the pulses and
 *     recomputes the backward chain itself, not normalised (everything is linear in chi, the stopping rule is relative).
 *   - The directions are a grid axis of the kernels (forward grid (K, nv), backward grid (K, L, nv)); a direction's result
 *     does not depend on nv or on the launch groups, bit for bit, and two calls give the same bits.  The storage is
 *     allocated by the first call, grows with nv in launch groups under the memory budget of grape_hvp (GRAPE_HVP_DIRS=<n>,
 *     read at create, sets the group size) and is freed by grape_destroy.
 *   - It owns its buffers and leaves the timing events and the statistics alone: after it grape_open_time_gradient,
 *     grape_get_tau_grads, grape_get_work, grape_get_timings and grape_get_storage(0) return what they returned before and
 *     a grape_eval is bit for bit what it was.
 *   - Series: m = ceil(beta_n dt_n / theta) sub-steps with the beta_n and theta of the gradient (B does not enter beta); all
 *     chains carry over between sub-steps; a series stops when EVERY chain has ||term||_F <= prop_tolerance ||sum||_F (a chain
 *     that is identically zero counts as converged), after at most 200 terms -- beyond that GRAPE_ERR_TAYLOR, and the
 *     handle stays usable.
 *   - GRAPE_ERR_INVALID with a message that names the reason, the handle stays usable: h == NULL (message:
 *     grape_last_error(NULL)), nv <= 0, V == NULL, HV == NULL; a closed handle (use grape_hvp); a split-phase shard
 *     (K < K_total); a handle without targets; no valid forward state (no evaluation yet, the last one failed,
 *     grape_set_tlist came since, or the last call was grape_eval_batch).  A caller-supplied chi (grape_backward_chi) is
 *     out of scope: it would need the caller's chi'(T). */
int grape_open_hvp(grape_handle *h, int nv, const double *V, double *HV);

/* What the last grape_open_hvp of this handle did, in the slots of grape_get_hvp_info: [0] series terms and [1] (sub-)steps
 * summed over the workgroups of both sweeps (K nv forward and K L nv backward workgroups, N_T steps each when no interval is
 * cut);  [2] directions per launch group;  [3] bytes of HVP storage the handle holds;  [4] milliseconds of the last call
 * (host wall time, copies included);  [5] the series terms of the tangent forward sweeps, [6] of the backward sweeps
 * ([0] = [5] + [6]).  Returns the number of entries written (at most n); GRAPE_ERR_INVALID for a closed handle. */
int grape_get_open_hvp_info(grape_handle *h, double *out, int n);

/* grape_open_hvp in two halves, cut at its one cross-trajectory dependency (entry points only, the ABI version stays 7;
 * csrc/grape_lindblad_hvp_split.hip.h).  What grape_open_hvp refuses -- a trajectory shard (K < K_total) and a
 * caller's functional, handles without targets included -- goes through these, as the gradient goes through grape_forward +
 * grape_backward / grape_backward_chi.  grape_open_hvp itself and its refusals are unchanged.  The semantics are those of
 * grape_hvp_forward / grape_hvp_backward / grape_hvp_backward_chi, with matrices for states.
 *
 * grape_open_hvp_forward: the tangent forward sweep of grape_open_hvp for nv directions V [nv][L*N_T] at the pulses of the
 * last forward half.  It leaves rho'_k(t_n) of ALL nv directions on the device and returns, each where the pointer is not NULL,
 *     dtau  [nv][K] complex       tau'_k = <<sigma_k | rho'_k(T)>>
 *     dsums [nv][2]               sum over THIS handle's k of w_k tau'_k -- what the host all-reduces between the halves
 *     drhoT [nv][K][N*N] complex  rho'_k(T), column-major (what a caller's chi' is formed from)
 * It needs what grape_open_hvp needs: a successful forward half on the current grid.  On a handle without targets dtau and
 * dsums come back NaN, as tau does.
 *
 * grape_open_hvp_backward: the built-in functional.  f_total is the all-reduced sum_k w_k tau_k (as for grape_backward),
 * df_total [nv][2] the all-reduced dsums.  It uses K_total and the handle's weights.  On an unsharded handle
 * grape_open_hvp_forward + grape_open_hvp_backward(grape_get_sums()[0:2], dsums) gives the bits of grape_open_hvp.
 *
 * grape_open_hvp_backward_chi: a caller's functional.  chi [K][N*N] complex = chi_k(T) as for grape_backward_chi on an open
 * handle, dchi [nv][K][N*N] its derivative along V[j] (both column-major; not normalised, no chi_min_norm guard: everything
 * is linear in chi).  It reads neither targets, weights, tau, f nor the functional.
 *
 *   - HV [nv][L*N_T] is the sum over this handle's trajectories: the full product when K == K_total, otherwise the partial
 *     sum the caller all-reduces like G.
 *   - A backward half needs a successful grape_open_hvp_forward with the same nv since the last of: any forward evaluation,
 *     grape_set_tlist, grape_eval_batch, grape_open_set_running_cost, grape_open_hvp (it shares the tangent storage and
 *     overwrites it).  Otherwise GRAPE_ERR_INVALID with a message that names which of these came between; the handle stays
 *     usable.  Any number of backward halves, of either kind, may follow one forward half.  grape_open_eval_batch,
 *     grape_open_time_gradient and a backward half of the gradient touch none of its storage and do not invalidate it.
 *   - All nv directions stay resident between the halves: an nv beyond the storage budget of grape_open_hvp (8 GB, half of
 *     the free memory) or beyond GRAPE_HVP_DIRS is GRAPE_ERR_INVALID, the message names the largest nv that fits; the caller
 *     loops.  What only the split calls need is allocated by the first of them, in a store of its own; a handle that never
 *     makes a split call allocates, and reports in grape_get_open_hvp_info[3], what it did before.
 *   - A direction's result does not depend on nv or on its position, and two calls give the same bits.  Nothing an
 *     evaluation, grape_open_time_gradient, grape_open_eval_batch or a getter reads is touched.
 *   - grape_get_open_hvp_info: after a forward half [5] = [0] = its series terms and [6] = 0; after a backward half [6] and
 *     [0] = [5] + [6]; [1] the (sub-)steps of both halves; [4] the milliseconds of the last call.
 *   - A series that does not converge within 200 terms: GRAPE_ERR_TAYLOR, as in grape_open_hvp; the handle stays usable.
 *   - GRAPE_ERR_INVALID with a message that names the reason, before the first HIP call: h == NULL (message:
 *     grape_last_error(NULL)); a NULL V / HV / chi / dchi / f_total / df_total; nv <= 0; a closed handle (grape_hvp_forward,
 *     grape_hvp_backward, grape_hvp_backward_chi are the calls for one); a state running cost set by
 *     grape_open_set_running_cost; grape_open_hvp_backward on a handle without targets (grape_open_hvp_backward_chi is the
 *     route). */
int grape_open_hvp_forward(grape_handle *h, int nv, const double *V, double *dtau, double *dsums, double *drhoT);
int grape_open_hvp_backward(grape_handle *h, int nv, const double f_total[2], const double *df_total, double *HV);
int grape_open_hvp_backward_chi(grape_handle *h, int nv, const double *chi, const double *dchi, double *HV);

/* P pulse vectors through the problem of one open-system handle, side by side (grape_create_open; entry points only, the
 * ABI version stays 7; csrc/grape_lindblad_batch.hip.h).  Arguments as grape_eval_batch:
 *   pulsevals [P][L*N_T] control-major per set;  J [P];  G NULL (forward half only) or [P][L*N_T];  tau NULL or [P][K] complex.
 * Element p is what grape_eval(h, pulsevals + p*L*N_T, ...) returns, to rounding.  An evaluation on such a handle is a latency
 * chain on K and K L of the 256 CUs whose time does not depend on K; here the sets are a grid axis of the kernels (forward
 * grid (K, Pg), backward grid (K, L, Pg)), so up to floor(256 / (K L)) evaluations cost about the time of one.
 *   - There is no route rule: P = 1 runs the same kernels.  A set's result does not depend on P, on its neighbours, on its
 *     position or on how P is cut into launch groups, bit for bit, and two calls give the same bits.  The kernels have no
 *     dependency between workgroups: any group size is legal, K L Pg far above the number of CUs included.
 *   - The call owns every per-set buffer (pulses, stored states, workspaces, tau and sums, ||chi||, tau_grads, G, flags,
 *     statistics): allocated by the first call, growing with P in launch groups under the memory budget of grape_open_hvp
 *     (GRAPE_OPEN_BATCH_SETS=<n>, read by grape_create_open, sets the group size), freed by grape_destroy.  It shares only the
 *     static data of the handle, the current time grid (grape_set_tlist is honoured) and the stream.  The last ordinary
 *     evaluation stays defined across the call: grape_open_time_gradient, grape_open_hvp, grape_get_tau_grads,
 *     grape_get_storage(0), grape_get_work, grape_get_timings and grape_get_sums return what they returned before, and a
 *     grape_eval afterwards is bit for bit what it was.  (grape_eval_batch on an open handle stays the loop over grape_eval
 *     it was, bit for bit, and does invalidate that state.)
 *   - No memory for even one set: GRAPE_ERR_HIP with a message that names the size; nothing is left allocated.
 *   - Flags are per set.  If a set raises GRAPE_ERR_TAYLOR or GRAPE_ERR_CHI_NORM the call returns the status of the lowest such
 *     p and grape_last_error names it ("pulse set p: ..."); the outputs are unspecified, the handle stays usable.
 *   - GRAPE_ERR_INVALID with a message that names the reason, before the first HIP call, the handle stays usable: h == NULL
 *     (message: grape_last_error(NULL)), P <= 0, pulsevals == NULL, J == NULL; a closed handle (use grape_eval_batch); a
 *     split-phase shard (K < K_total); a handle without targets.  A caller-supplied chi and final states per set are out of
 *     scope. */
int grape_open_eval_batch(grape_handle *h, int P, const double *pulsevals, double *J, double *G, double *tau);

/* What the last grape_open_eval_batch of this handle did: [0] sets per launch group;  [1] number of groups;  [2] bytes of batch
 * storage the handle holds;  [3] milliseconds of the last call (host wall time, copies included);  [4] series terms of the
 * forward sweeps, [5] of the backward sweeps (0 after a call without G), [6] (sub-)steps, each summed over all workgroups of
 * the call.  Returns the number of entries written (at most n); GRAPE_ERR_INVALID for a closed handle. */
int grape_get_open_batch_info(grape_handle *h, double *out, int n);

/* State running costs on open-system handles (grape_create_open; entry points only, the ABI version stays 7;
 * csrc/grape_lindblad_rc.hip.h): J = J_T + lambda_b J_b with J_b = sum_k sum_{n=0}^{N_T} wq_n g_b(rho_k(t_n)) and the
 * trapezoid weights wq of optimize.jl:727-750 on the current grid.  grape_create_open with Dpen and grape_backward_xi on an
 * open handle stay the refusals they are.
 *
 * grape_open_set_running_cost installs the built-in family g_b(rho) = Re tr(D rho) -- the population of leakage levels for a
 * projector D; <Psi|D|Psi> of the closed path for a pure rho -- or removes it (D == NULL or lambda_b == 0).
 *   D: [N*N] shared (d_per_traj == 0) or [K][N*N], column-major complex, Hermitian in the intended use.  In the reference's
 *   convention dg_b = -2 Re <<xi | d rho>> the family has the constant xi_k = -D_k^dagger / 2.
 *   - The call waits for work in flight, uploads -D^dagger / 2 and (re)computes wq.  Like grape_set_tlist it makes the next call
 *     a forward evaluation; it may be repeated, e.g. for a continuation in lambda_b.  grape_set_tlist recomputes wq.
 *   - While a cost is set grape_eval, grape_forward, grape_backward, grape_backward_chi and grape_eval_batch (the loop over
 *     grape_eval) include it: grape_get_sums[4] = sum_k J_b,k of this handle's trajectories, J of grape_eval is
 *     J_T + lambda_b J_b, the backward half adds lambda_b wq_{N_T} xi_k(T) to chi_k(T) BEFORE the norm, the chi_min_norm guard and
 *     the normalisation, and (lambda_b wq_n / ||chi_k(T)||) xi_k to chi_k(t_n) for 0 < n < N_T, once per interval.
 *   - After removal every result is bit for bit what a handle that never had a cost gives: such a handle launches the
 *     kernels it always did.
 *   - Not carried, and refused with a message that names the running cost (the handle stays usable): grape_open_hvp and
 *     grape_open_eval_batch while a cost is set; grape_open_time_gradient after a backward half that carried a cost of either
 *     form (a later backward half without one makes it answer again).
 *   - GRAPE_ERR_INVALID, the handle stays usable: h == NULL (message: grape_last_error(NULL)); a closed handle; D != NULL with a
 *     non-finite lambda_b.  An allocation failure is GRAPE_ERR_HIP with a message that names the size. */
int grape_open_set_running_cost(grape_handle *h, const double *D, int d_per_traj, double lambda_b);

/* The backward half with the inhomogeneity of an ARBITRARY state running cost: the arguments of grape_backward_xi with matrices
 * for states.  xi [K][N_T+1][N*N] column-major, xi_k(t_n) defined by dg_b = -2 Re <<xi | d rho>> and evaluated by the caller on
 * grape_get_storage(0) (entry n = 0 is not read; g_b = -tr rho^2 has xi = rho);  chi NULL (the handle's functional with f_total)
 * or [K][N*N], the caller's chi_k(T);  G [L*N_T] = the gradient of J_T + lambda_b J_b.  J_b itself stays the caller's.  The call
 * overrides a built-in cost for this backward half.  The xi buffer on the device is allocated by the first call and freed by
 * grape_destroy; xi is staged one trajectory at a time.
 *   GRAPE_ERR_INVALID with a message that names the reason, the handle stays usable: h == NULL; a closed handle (use
 *   grape_backward_xi); xi == NULL or G == NULL; chi == NULL with f_total == NULL or on a handle without targets; no forward half
 *   since grape_create_open, grape_set_tlist or grape_open_set_running_cost. */
int grape_open_backward_xi(grape_handle *h, const double f_total[2], const double *chi, const double *xi, double lambda_b,
                           double *G);

/* Expectation values of operator observables on the stored forward states of the last evaluation, computed on the device
 * (entry points only, the ABI version stays 7; csrc/grape_expect.hip.h).  The reference hands `observables` to a
 * callback after every prop_step! of the forward sweep (src/optimize.jl:733-737); here the sweep has run and K (N_T+1) M numbers
 * come back instead of the K (N_T+1) N states of grape_get_storage(0).
 *   ops: [M][N*N] complex column-major, one set for all trajectories (ops_per_traj == 0), or [K][M][N*N] (== 1); 1 <= M <= 16.
 *        The operators need not be Hermitian.
 *   out: [K][N_T+1][M] complex; entry n belongs to t_n, n = 0 is the initial state.
 *        closed handle: out[k][n][m] = <Psi_k(t_n)| O_m |Psi_k(t_n)>;  open handle (grape_create_open, N = d):
 *        out[k][n][m] = tr(O_m rho_k(t_n)).  Values are in the caller's frame: a balanced handle stores D^-1 Psi and the upload
 *        forms D O D (exact, powers of two), as Dpen is treated.
 *   - It reads only the stored forward states, so it serves every handle that has them: all closed sizes and routes, with or
 *     without Dpen or targets, split-phase shards (the local K trajectories), several devices behind one handle (per shard,
 *     ops sliced like out when ops_per_traj == 1), open handles with or without a running cost.
 *   - Valid after any successful call that ran the forward half on the current grid (grape_eval with or without G,
 *     grape_forward, grape_forward_device; after a device-pointer call on a foreign stream it waits for the device).
 *   - GRAPE_ERR_INVALID with a message that names the call and the reason, before the first HIP call, the handle unchanged and
 *     usable: h == NULL (message: grape_last_error(NULL)); ops == NULL; out == NULL; M <= 0; M > 16; ops_per_traj not 0 or 1; no
 *     evaluation yet; the last evaluation failed; grape_set_tlist, grape_open_set_running_cost or grape_eval_batch since
 *     (grape_open_eval_batch does not invalidate the store).
 *   - The operators on the device and the result are buffers of the call: allocated by the first call through the handle's
 *     allocator, grown on demand, freed by grape_destroy.  A failed allocation is GRAPE_ERR_HIP with the size in the message and
 *     nothing is left allocated.  Nothing an evaluation, a getter, the time gradient, a Hessian-vector product or a batch reads
 *     or writes is touched: a grape_eval afterwards is bit for bit what it was.
 *   - Two calls give the same bits; the value of one observable does not depend on M, on its position in ops or on the other
 *     operators, bit for bit (no atomics, every reduction in a fixed order). */
int grape_expect(grape_handle *h, int M, const double *ops, int ops_per_traj, double *out);

/* What the last grape_expect of this handle did: [0] its M;  [1] bytes this feature holds on the device;  [2] milliseconds of the
 * last call (host wall time, copies included);  [3] flop of the matrix instructions the kernel executed (0 on an open handle,
 * whose kernel is element-wise).  Returns the number of entries written (at most n). */
int grape_get_expect_info(grape_handle *h, double *out, int n);

const char *grape_last_error(grape_handle *h); /* h may be NULL: error of the last failed create */
int grape_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GRAPE_HIP_H */
