"""Inputs of tests/test_gpu_sequences.py: eight small problems, and for each the pulses, directions, boundary
states and running-cost data of every step of the script one long-lived handle is driven through.  numpy / scipy only, so
that tests/test_sequence_inputs.py can check the inputs without a GPU.

Every step uses pulses of its own, x_i = x_0 + 1e-2 * noise_i.  No step changes the time grid."""
import numpy as np
from scipy.linalg import expm

from grape_jl_amd import synth

# id: N, L, N_T, K (each N_T leaves a partial last derivative batch of 16), generators, functional
CASES = {
    "s16h": dict(N=16, L=1, N_T=37, K=3, herm=True, f=0),                  # batched kernels, deriv_kernel<16>
    "s10g": dict(N=10, L=2, N_T=21, K=2, herm=False, f=1, skew=3),         # padding 10 -> 16, balanced frame
    "s32h": dict(N=32, L=2, N_T=37, K=3, herm=True, f=2),                  # deriv_kernel<32>
    "s20g": dict(N=20, L=2, N_T=21, K=2, herm=False, f=0),                 # NP = 32 padded
    "s40h": dict(N=40, L=2, N_T=37, K=2, herm=True, f=0),                  # NP = 48, deriv2_kernel
    "s64h": dict(N=64, L=2, N_T=21, K=2, herm=True, f=0),                  # expm_t16_asm, deriv2_kernel + economized series
    "s57p": dict(N=57, L=2, N_T=21, K=2, herm=True, f=0, per_traj=True),   # expm_t16p_asm
    "s64g": dict(N=64, L=2, N_T=21, K=2, herm=False, f=0),                 # expm_t18g_asm
}
# the shape of the getter defect: tools/hvp_ab.py case C2, where it was seen
PART_A = dict(N=16, L=1, N_T=500, K=32)
N_PULSES = 40          # pulse vectors a script may draw
LAMBDA_B = 0.3
_cache = {}


def _seed(cid):
    return 5000 + sum(map(ord, cid))


def problem(cid):
    """the problem of a case: H0, Hc, tlist, psi0, target, weights, functional, pulsevals (= x_0); computed once"""
    if cid in _cache:
        return _cache[cid]
    c = CASES[cid]
    N, L, N_T, K, seed = c["N"], c["L"], c["N_T"], c["K"], _seed(cid)
    pr = synth.make_problem(N, L, N_T, K, seed=seed, hermitian=c["herm"])
    if c.get("per_traj"):
        pr["Hc"] = np.stack([np.stack([synth.gue(synth.subseed(seed, 500 + 10 * k + l), N) for l in range(L)]) for k in range(K)])
    if c.get("skew"):      # S H S^-1 with S = diag(2^e): exact, and the balancing of the handle is not the identity
        sk = c["skew"]
        e = (synth.splitmix64(synth.subseed(seed, 11), N) % np.uint64(2 * sk + 1)).astype(np.int64) - sk
        e[0], e[-1] = -sk, sk
        S = 2.0 ** e
        pr["H0"] = S[:, None] * pr["H0"] / S[None, :]
        pr["Hc"] = S[:, None] * pr["Hc"] / S[None, :]
        pr["psi0"] = pr["psi0"] * S[None, :]
        pr["psi0"] /= np.linalg.norm(pr["psi0"], axis=1, keepdims=True)
    pr["weights"] = 0.5 + synth.uniform01(synth.subseed(seed, 8100), K)
    pr["functional"] = c["f"]
    # targets with O(1) overlaps: the normalised Psi_k(T) of the pulses 0.8 x_0
    eps = 0.8 * pr["pulsevals"].reshape(L, N_T)
    psi = pr["psi0"].copy()
    for k in range(K):
        Hc = pr["Hc"][k] if pr["Hc"].ndim == 4 else pr["Hc"]
        for n in range(N_T):
            H = pr["H0"][k] + sum(eps[l, n] * Hc[l] for l in range(L))
            psi[k] = expm(-1j * (pr["tlist"][n + 1] - pr["tlist"][n]) * H) @ psi[k]
    pr["target"] = psi / np.linalg.norm(psi, axis=1, keepdims=True)
    _cache[cid] = pr
    return pr


def pulses(cid, i):
    """x_i = x_0 + 1e-2 noise_i (x_0 itself for i = 0)"""
    pr = problem(cid)
    assert 0 <= i < N_PULSES
    if i == 0:
        return pr["pulsevals"].copy()
    return pr["pulsevals"] + 1e-2 * synth.normal(synth.subseed(_seed(cid), 7000 + i), pr["pulsevals"].size)


def directions(cid, nv=2):
    pr = problem(cid)
    n = pr["pulsevals"].size
    return 2.0 * synth.uniform01(synth.subseed(_seed(cid), 9100), nv * n).reshape(nv, n) - 1.0


def penalty(cid):
    """D = A A^+ / N, A complex Ginibre: the state running cost g_b = <Psi|D|Psi> of step 6"""
    N = CASES[cid]["N"]
    z = synth.normal(synth.subseed(_seed(cid), 9200), 2 * N * N)
    A = (z[0::2] + 1j * z[1::2]).reshape(N, N)
    D = A @ A.conj().T / N
    return 0.5 * (D + D.conj().T)


def caller_chi(cid, psiT):
    """boundary states of a functional the library does not know: chi_k = 0.25 conj(Psi_k(T)) + 0.1 target_k"""
    return 0.25 * np.conj(psiT) + 0.1 * problem(cid)["target"]


def part_a_problem():
    from grape_jl_amd.synth import BASE_SEED
    a = PART_A
    return synth.make_problem(a["N"], a["L"], a["N_T"], a["K"], seed=BASE_SEED ^ 2)


def part_a_pulses(i):
    pr = part_a_problem()
    return pr["pulsevals"] + (0.0 if i == 0 else 1e-2) * synth.normal(synth.subseed(77, 7000 + i), pr["pulsevals"].size)


# The script (tests/test_gpu_sequences.py runs it, DESIGN.md 23 lists it): entry points in the order one handle makes them.
# No entry is grape_set_tlist.
SCRIPT = (
    ("eval",) * 4,
    ("final_states", "sums", "storage0", "storage1", "tau_grads", "propagator", "work", "timings", "time_gradient", "eval"),
    ("eval_no_gradient", "eval"),
    ("forward", "final_states", "backward_chi", "time_gradient", "eval"),
    ("forward", "sums", "backward", "eval"),
    ("forward", "storage0", "backward_xi", "eval"),
    ("eval", "hvp", "eval"),
    ("eval_batch", "eval"),
    ("set_fused_sweeps_off", "eval", "set_fused_sweeps_on", "eval"),
    ("eval",) * 12,
)
GETTERS = ("final_states", "sums", "storage0", "storage1", "tau_grads", "propagator", "work", "timings", "time_gradient")
