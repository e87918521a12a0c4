"""Proof of tests/open_hvp_reference.py on the CPU: the forward-over-forward reference of grape_open_hvp against Richardson-
extrapolated central differences of the gradient of open_reference.evaluate, against the closed reference hvp_reference.evaluate on
the vectorised problem, double against long double, two sub-step thresholds against each other, the symmetry of the Hessian, the
numpy transcription of the kernels' block recursion -- and that the shared comparison refuses deliberately wrong references."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hvp_reference as hr  # noqa: E402
import open_helpers as oh  # noqa: E402
import open_hvp_reference as ohr  # noqa: E402
import open_reference as orf  # noqa: E402
import open_time_reference as otr  # noqa: E402
from open_hvp_reference import RE, SM, SS  # noqa: E402

# Richardson-extrapolated central differences of G, h = 1e-2 and h / 2: the h^2 term cancels, h^4 G^(5) / 20 ~ 1e-9 |G^(5)| is
# left, and the rounding of G (1e-16) / h ~ 1e-14.  Worst measured deviation over the twelve cases below, relative to
# ||Hv||_inf: 8.8e-10; asserted at ten times that, and never looser than 1e-6 (the rule of DESIGN.md 14).
FD_MEASURED = 8.8e-10
FD_BOUND = min(10 * FD_MEASURED, 1e-6)


def _case(d, J, functional, **kw):
    c = dict(d=d, J=J, L=2, K=2, N_T=4, functional=functional, weights=True, shape=True, nonuniform=True)
    c.update(kw)
    return otr.build_case(c)


@pytest.mark.parametrize("functional", [SM, SS, RE])
@pytest.mark.parametrize("d,J", [(3, 0), (3, 2), (5, 0), (5, 2)])
def test_against_richardson_differences_of_the_reference_gradient(d, J, functional):
    pr = _case(d, J, functional)
    x = pr["pulsevals"]
    V = ohr.directions(100 * d + J, 2, x.size)
    want = ohr.evaluate(pr, x, V, functional)
    ev = orf.evaluate(pr, x, functional)
    assert abs(want["J"] - ev["J"]) <= 1e-14 and np.abs(want["G"] - ev["G"]).max() <= 1e-14 and np.abs(want["tau"] - ev["tau"]).max() <= 1e-14

    def diff(h, v):
        return (orf.evaluate(pr, x + h * v, functional)["G"] - orf.evaluate(pr, x - h * v, functional)["G"]) / (2 * h)

    size = float(np.abs(want["Hv"]).max())
    assert size >= 1e-3
    for j, v in enumerate(V):
        fd = (4 * diff(0.005, v) - diff(0.01, v)) / 3
        rel = float(np.abs(fd - want["Hv"][j]).max()) / size
        print(dict(d=d, J=J, functional=functional, direction=j, rel=rel))
        assert rel <= FD_BOUND


@pytest.mark.parametrize("J", [0, 3])
@pytest.mark.parametrize("d,functional", [(2, SM), (3, SS), (4, RE)])
def test_against_the_closed_reference_on_the_vectorised_problem(d, J, functional):
    """operators per trajectory, non-Hermitian drift and states: hvp_reference (scipy expm, Frechet derivatives, the 4 x 4 block
    matrix) on the d^2-dimensional problem of open_helpers.vectorised"""
    pr = _case(d, J, functional, N_T=3, cops_per_traj=J > 0, hc_per_traj=True, hermitian=False, non_hermitian_states=0.3)
    x = pr["pulsevals"]
    V = ohr.directions(200 * d + J, 2, x.size)
    want = ohr.evaluate(pr, x, V, functional)
    v = oh.vectorised(pr)
    closed = hr.evaluate(dict(H0=v["H0"], Hc=v["Hc"], psi0=v["psi0"], target=v["target"], tlist=pr["tlist"], weights=pr["weights"],
                              shape=pr["shape"]), x, V, functional)
    fig = dict(dJ=abs(closed["J"] - want["J"]), dG=np.abs(closed["G"] - want["G"]).max(), dHv=np.abs(closed["Hv"] - want["Hv"]).max())
    print(d, J, functional, fig)
    assert max(fig.values()) <= 1e-12


@pytest.mark.parametrize("d,J,functional", [(4, 2, SM), (17, 3, SS)])
def test_long_double_and_two_substep_thresholds(d, J, functional):
    pr = _case(d, J, functional, N_T=2 if d == 17 else 3, L=2)
    x = pr["pulsevals"]
    V = ohr.directions(300 + d, 2 if d == 4 else 1, x.size)
    a = ohr.evaluate(pr, x, V, functional, theta=1.0)
    b = ohr.evaluate(pr, x, V, functional, theta=0.4)
    c = ohr.evaluate(pr, x, V, functional, dtype=np.clongdouble, theta=1.0)
    size = max(1.0, float(np.abs(a["Hv"]).max()))
    fig = dict(theta=float(np.abs(a["Hv"] - b["Hv"]).max()), long=float(np.abs(a["Hv"] - np.asarray(c["Hv"], dtype=float)).max()))
    print(d, fig)
    assert c["Hv"].dtype == np.longdouble
    assert max(fig.values()) <= 1e-13 * size


@pytest.mark.parametrize("functional", [SM, SS, RE])
def test_the_hessian_is_symmetric(functional):
    pr = _case(5, 2, functional)
    x = pr["pulsevals"]
    V = ohr.directions(77, 3, x.size)
    Hv = ohr.evaluate(pr, x, V, functional)["Hv"]
    A = V @ Hv.T          # A[i][j] = v_i . H v_j
    scale = float(np.abs(A).max())
    print(functional, dict(asym=float(np.abs(A - A.T).max()), scale=scale))
    assert scale >= 1e-3
    assert np.abs(A - A.T).max() <= 1e-12 * scale


@pytest.mark.parametrize("d,J,functional,long_step", [(4, 2, SM, None), (5, 0, SS, None), (6, 3, RE, 6.0), (17, 2, SM, 4.0)])
def test_the_block_recursion_of_the_kernels(d, J, functional, long_step):
    """the adjoint form of csrc/grape_lindblad_hvp.hip.h, an interval of several sub-steps included"""
    pr = _case(d, J, functional, N_T=3, long_step=long_step, nonuniform=long_step is None, K=3 if d == 4 else 2)
    x = pr["pulsevals"]
    V = ohr.directions(400 + d, 2, x.size)
    V[0].reshape(2, 3)[:, 0] = 0.0      # a direction that is zero on one interval: an identically zero chain
    want = ohr.evaluate(pr, x, V, functional)
    got, msub = ohr.block_recursion(pr, x, V, functional, want_substeps=True)
    size = max(1.0, float(np.abs(want["Hv"]).max()))
    print(d, dict(dev=float(np.abs(got - want["Hv"]).max()), substeps=msub.tolist()))
    if long_step:
        assert msub[:, 1].min() >= 2
    assert np.abs(got - want["Hv"]).max() <= 1e-13 * size


@pytest.fixture(scope="module")
def refusal_case():
    """weights [0.5, 1.0, 1.5], a shape that differs between the controls, collapse operators, O(1) signals"""
    pr = _case(4, 2, SM, N_T=3, K=3)
    x = pr["pulsevals"]
    V = ohr.directions(500, 2, x.size)
    return pr, x, V, {f: ohr.evaluate(pr, x, V, f) for f in (SM, SS)}


def test_the_comparison_accepts_the_block_recursion(refusal_case):
    pr, x, V, want = refusal_case
    for f in (SM, SS):
        ohr.assert_open_hvp_agrees(ohr.block_recursion(pr, x, V, f), want[f], f"block recursion, functional {f}")


@pytest.mark.parametrize("wrong", ohr.WRONG)
def test_the_comparison_refuses_a_wrong_reference(refusal_case, wrong):
    pr, x, V, want = refusal_case
    for f in (SM,) if wrong == "zero_chi_prime" else (SM, SS):
        bad = ohr.block_recursion(pr, x, V, f, wrong=wrong)
        with pytest.raises(AssertionError):
            ohr.assert_open_hvp_agrees(bad, want[f], wrong)


def test_the_comparison_refuses_small_signals(refusal_case):
    """the conditions on the reference alone: a reference whose signals sit at the floor of the bound is not a reference"""
    pr, x, V, want = refusal_case
    small = dict(want[SM], Hv=1e-6 * want[SM]["Hv"])
    with pytest.raises(AssertionError):
        ohr.assert_open_hvp_agrees(small["Hv"], small, "small Hv")
    with pytest.raises(AssertionError):
        ohr.assert_open_hvp_agrees(want[SM]["Hv"], dict(want[SM], tau=0.01 * want[SM]["tau"]), "small tau")
