"""tests/open_hessian_reference.py (the adjoint form on the stored states) against the forward-over-forward reference of
tests/open_hvp_reference.py with the identity as directions -- another formula altogether: no adjoint chain, no stored state,
no fan --, its symmetry, and the proof that the shared comparison refuses wrong references.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_hessian_reference as ohs  # noqa: E402
import open_hvp_reference as ohr  # noqa: E402
import open_time_reference as otr  # noqa: E402
from open_hessian_reference import RE, SM, SS  # noqa: E402

GRID = dict(weights=True, shape=True, nonuniform=True)
SHAPES = {
    "d3-J2-L2-NT4-K2-sm": dict(d=3, J=2, L=2, K=2, N_T=4, functional=SM, **GRID),
    "d5-J0-L2-NT3-K2-ss": dict(d=5, J=0, L=2, K=2, N_T=3, functional=SS, nonuniform=True),
    "d3-J2-L3-NT4-K2-re": dict(d=3, J=2, L=3, K=2, N_T=4, functional=RE, **GRID),
    "d5-J2-L2-NT3-K3-ss": dict(d=5, J=2, L=2, K=3, N_T=3, functional=SS, **GRID),
    "d5-J2-L1-NT4-K2-sm-general-drift": dict(d=5, J=2, L=1, K=2, N_T=4, functional=SM, hermitian=False, non_hermitian_states=0.3,
                                             cops_per_traj=True, nonuniform=True),
}

# the largest relative deviation ||H - H_fof||_inf / ||H||_inf measured over SHAPES (complex128, both series to 1e-18)
MEASURED_REL = 1.4e-15
BAR_REL = min(10 * MEASURED_REL, 1e-12)     # ten times that, never looser than the bar of tests/test_hessian_reference.py


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, spec in SHAPES.items():
        pr = otr.build_case(spec)
        out[name] = (pr, ohs.evaluate(pr, pr["pulsevals"], pr["functional"]))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_against_forward_over_forward_with_identity_directions(cases, name):
    pr, want = cases[name]
    ohr.assert_order_one(dict(tau=want["tau"], G=want["G"], Hv=want["H"]))
    P = pr["pulsevals"].size
    other = ohr.evaluate(pr, pr["pulsevals"], np.eye(P), pr["functional"])
    scale = float(np.abs(other["Hv"]).max())
    dev = float(np.abs(want["H"] - other["Hv"]).max())
    print(name, dict(dH=dev, rel=dev / scale, H_max=scale, dG=float(np.abs(want["G"] - other["G"]).max())))
    assert abs(want["J"] - other["J"]) <= 1e-14
    assert np.abs(want["tau"] - other["tau"]).max() <= 1e-14
    assert np.abs(want["G"] - other["G"]).max() <= 1e-12 * max(np.abs(other["G"]).max(), 1.0)
    assert dev <= BAR_REL * scale


@pytest.mark.parametrize("name", list(SHAPES))
def test_reference_is_symmetric(cases, name):
    _, want = cases[name]
    H = want["H"]
    assert np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()


# (mutation, the shapes it is tried on): the boundary term under sm and under ss (it vanishes under re); the dissipator of the
# carried columns where there is one and the fan carries (N_T >= 3); the last weight where it is not 1 (K = 3)
MUTATIONS = [("drop_diagonal_blocks", "d3-J2-L2-NT4-K2-sm"), ("drop_boundary", "d3-J2-L2-NT4-K2-sm"), ("drop_boundary", "d5-J2-L2-NT3-K3-ss"),
             ("fan_one_interval_too_many", "d3-J2-L2-NT4-K2-sm"), ("no_dissipator_in_columns", "d3-J2-L3-NT4-K2-re"),
             ("no_dissipator_in_columns", "d5-J2-L2-NT3-K3-ss"), ("k_for_k_total", "d5-J0-L2-NT3-K2-ss"),
             ("k_for_k_total", "d3-J2-L3-NT4-K2-re"), ("ignore_last_weight", "d5-J2-L2-NT3-K3-ss")]


@pytest.mark.parametrize("wrong,name", MUTATIONS)
def test_the_comparison_refuses_wrong_references(cases, wrong, name):
    """every deliberate mistake moves H by far more than the bound of assert_open_hessian_agrees.  K for K_total shows only
    where the two differ: there the right reference is that of a problem twice as large (K_total = 2 K)"""
    pr, want = cases[name]
    assert wrong in ohs.WRONG
    f, K = pr["functional"], pr["H0"].shape[0]
    right = want if wrong != "k_for_k_total" else ohs.evaluate(pr, pr["pulsevals"], f, K_total=2 * K)
    bad = ohs.evaluate(pr, pr["pulsevals"], f, K_total=2 * K if wrong == "k_for_k_total" else None, wrong=wrong)
    ohs.assert_open_hessian_agrees(right["H"], right, "right")
    with pytest.raises(AssertionError):
        ohs.assert_open_hessian_agrees(bad["H"], right, wrong)
