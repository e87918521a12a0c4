"""The reference of the Hessian tests (tests/hessian_reference.py) proved on the CPU: against tests/hvp_reference.py with the
identity for directions (itself proved against finite differences of the oracle, tests/test_hvp_reference.py), by its symmetry,
and by the shared comparison refusing deliberately wrong references.  No GPU, nothing of the product path.

Both references are double-precision restatements of the same derivative with different formulas (explicit Psi', chi' there;
seeds, fan and a closed boundary term here).  Their largest deviation over the five shapes below was measured as 2.2e-16 for
||H||_inf between 0.27 and 0.84; the bound is 1e-12 ||H||_inf.  At the lengths of the device test's long cases (300 and 2048
intervals, seven to nine columns each) it was 1.0e-15 at ||H||_inf = 0.81 and 2.2e-16 at 0.085, under the same bound."""
import numpy as np
import pytest

import hessian_reference as hs
import hvp_reference as hr

# (N, L, N_T, K, functional, controls per trajectory): all with weights, shape and a non-uniform grid
SHAPES = {
    "N3-L1-NT20-K2-sm": (3, 1, 20, 2, 0, False),
    "N5-L2-NT9-K2-ss-pertraj": (5, 2, 9, 2, 1, True),
    "N6-L3-NT11-K3-sm": (6, 3, 11, 3, 0, False),
    "N4-L4-NT5-K2-re": (4, 4, 5, 2, 2, False),
    "N5-L3-NT6-K2-ss": (5, 3, 6, 2, 1, False),
}


def problem(N, L, N_T, K, per_traj):
    from grape_jl_amd import synth
    seed = 77 + N
    pr = synth.make_problem(N, L, N_T, K, seed=seed)
    pr["pulsevals"] = 3.0 * pr["pulsevals"]
    if per_traj:
        pr["Hc"] = np.stack([np.stack([synth.gue(synth.subseed(seed, 500 + 10 * k + l), N) for l in range(L)]) for k in range(K)])
    u = synth.uniform01(synth.subseed(seed, 8100), N_T + L * N_T + K)
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(0.5 + u[:N_T])])
    pr["shape"] = 0.5 + 0.5 * u[N_T:N_T + L * N_T].reshape(L, N_T)
    pr["weights"] = 0.5 + u[N_T + L * N_T:]
    hr.order_one_targets(pr)
    return pr


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, (N, L, N_T, K, f, per_traj) in SHAPES.items():
        pr = problem(N, L, N_T, K, per_traj)
        out[name] = (pr, f, hs.evaluate(pr, pr["pulsevals"], f))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_against_the_hvp_reference_with_identity_directions(cases, name):
    pr, f, want = cases[name]
    hs.assert_order_one(want)
    P = pr["L"] * pr["N_T"]
    other = hr.evaluate(pr, pr["pulsevals"], np.eye(P), f)
    scale = np.abs(other["Hv"]).max()
    dev = np.abs(want["H"] - other["Hv"]).max()
    print(name, dict(dH=dev, H_max=scale, dG=np.abs(want["G"] - other["G"]).max()))
    assert abs(want["J"] - other["J"]) <= 1e-14
    assert np.abs(want["tau"] - other["tau"]).max() <= 1e-14
    assert np.abs(want["G"] - other["G"]).max() <= 1e-12 * max(np.abs(other["G"]).max(), 1.0)
    assert dev <= 1e-12 * scale


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_is_symmetric(cases, name):
    _, _, want = cases[name]
    H = want["H"]
    assert np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()


# the two longest cases of the device test's second table, under its names and seeds (tests/test_gpu_hessian.py imports
# without a GPU): 300 and 2048 intervals, where the comparison above stops at 20
LONG = ["N3-L2-NT300-K4-sm-strided-seeds", "N2-L1-NT2048-K1-re-two-intervals-per-seed"]


@pytest.mark.parametrize("name", LONG)
def test_reference_at_the_lengths_of_the_long_device_cases(name):
    """columns of H against the hvp reference with the matching unit directions, where the device's launch plan changes
    (first and last column, q = 15 and 16, both sides of n = rows, one mid column), and the symmetry of the whole matrix"""
    import test_gpu_hessian as dev
    assert name in dev.LONG_CASES
    pr, f, want = dev.case(name)
    hs.assert_order_one(want)
    L, N_T, K = pr["L"], pr["N_T"], pr["K"]
    P, rows = L * N_T, dev.seed_rows(K, N_T)
    assert rows < N_T
    cols = dev.probe_columns(L, N_T, K)
    n_of = cols % N_T
    assert {0, P - 1} <= set(cols.tolist()) and {rows - 1, rows} <= set(n_of.tolist()) and 7 <= len(cols) <= 9
    E = np.zeros((len(cols), P))
    E[np.arange(len(cols)), cols] = 1.0
    other = hr.evaluate(pr, pr["pulsevals"], E, f)
    H = want["H"]
    scale = np.abs(H).max()
    dev_cols = np.abs(H[:, cols].T - other["Hv"]).max()
    print(name, dict(columns=cols.tolist(), dH=dev_cols, H_max=scale, asym=np.abs(H - H.T).max()))
    assert abs(want["J"] - other["J"]) <= 1e-14
    assert np.abs(want["tau"] - other["tau"]).max() <= 1e-14
    assert np.abs(want["G"] - other["G"]).max() <= 1e-12 * max(np.abs(other["G"]).max(), 1.0)
    assert dev_cols <= 1e-12 * scale
    assert np.abs(H - H.T).max() <= 1e-14 * scale


# (mutation, the shapes it is tried on): the boundary term under sm and under ss (it vanishes under re)
MUTATIONS = [("drop_diagonal_blocks", "N6-L3-NT11-K3-sm"), ("drop_boundary", "N6-L3-NT11-K3-sm"), ("drop_boundary", "N5-L3-NT6-K2-ss"),
             ("fan_one_interval_too_many", "N6-L3-NT11-K3-sm"), ("k_for_k_total", "N5-L2-NT9-K2-ss-pertraj"),
             ("k_for_k_total", "N4-L4-NT5-K2-re"), ("ignore_last_weight", "N6-L3-NT11-K3-sm")]


@pytest.mark.parametrize("wrong,name", MUTATIONS)
def test_the_comparison_refuses_wrong_references(cases, wrong, name):
    """every deliberate mistake moves H by far more than the bound of assert_hessian_agrees.  K for K_total shows only where
    the two differ: there the right reference is that of a problem twice as large (K_total = 2 K)"""
    pr, f, want = cases[name]
    assert wrong in hs.WRONG
    right = want["H"] if wrong != "k_for_k_total" else hs.evaluate(pr, pr["pulsevals"], f, K_total=2 * pr["K"])["H"]
    bad = hs.evaluate(pr, pr["pulsevals"], f, K_total=2 * pr["K"] if wrong == "k_for_k_total" else None, wrong=wrong)
    hs.assert_hessian_agrees(right, right, "right")
    with pytest.raises(AssertionError):
        hs.assert_hessian_agrees(bad["H"], right, wrong)
