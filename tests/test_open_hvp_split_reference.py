"""Proves tests/open_hvp_split_reference.py (the forward-over-forward reference with a caller's boundary, and the shared
comparison of the caller's route) on the CPU: the built-in functionals written as a boundary against
open_hvp_reference.evaluate, the Hilbert-Schmidt functional against Richardson-extrapolated central differences of the
reference's own G and J, double against long double, and the refusals of the shared comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_hvp_reference as ohr  # noqa: E402
import open_hvp_split_reference as osr  # noqa: E402
import open_time_reference as otr  # noqa: E402
from open_hvp_split_reference import RE, SM, SS  # noqa: E402

GRID = dict(weights=True, shape=True, nonuniform=True)

# measured on the cases below (printed by the tests); the assertions stand at ten times these
BUILTIN_HV_REL_MEASURED = 2.6e-16   # ||Hv_boundary - Hv_evaluate||_inf / ||Hv||_inf, largest of the twelve cases (d = 5, J = 3, ss)
BUILTIN_G_REL_MEASURED = 3.0e-15    # the same for G, relative to ||G||_inf (d = 2, J = 0, sm)
FD_HV_REL_MEASURED = 1.5e-12        # ||Hv - Richardson differences of G||_inf / ||Hv||_inf, larger of d = 3, 5 (d = 3)
FD_G_REL_MEASURED = 5.5e-11         # |G.v - Richardson differences of J| / |G.v|, larger of d = 3, 5 (d = 3, G.v = 2.4e-3)


def _case(d, J, functional=SM, K=2, **kw):
    return otr.build_case(dict(dict(d=d, J=J, L=2, K=K, functional=functional, **GRID), **kw))


@pytest.mark.parametrize("functional", [SM, SS, RE])
@pytest.mark.parametrize("d,J", [(2, 0), (2, 3), (5, 0), (5, 3)])
def test_builtin_functionals_as_a_boundary_reproduce_the_builtin_reference(d, J, functional):
    """The propagation is the same term for term (rho(T), tau' are EQUAL); the boundary contracts chi = c sigma with the stack
    where open_hvp_reference contracts sigma first and multiplies by c afterwards, so J, G, H v agree to rounding: measured
    2.6e-16 of ||Hv||_inf (3.0e-15 of ||G||_inf) at most, required below 1e-13, asserted at ten times the measured values."""
    pr = _case(d, J, functional)
    x = pr["pulsevals"]
    V = ohr.directions(31 * d + J, 2, x.size)
    want = ohr.evaluate(pr, x, V, functional)
    got = osr.evaluate_chi(pr, x, V, osr.builtin(pr["target"], functional, pr["weights"]))
    assert np.array_equal(got["dtau"], want["dtau"])
    tau = osr.inner(np.asarray(pr["target"]), got["rhoT"])
    assert np.array_equal(tau, want["tau"])
    size = float(np.abs(want["Hv"]).max())
    rel = float(np.abs(got["Hv"] - want["Hv"]).max()) / size
    relG = float(np.abs(got["G"] - want["G"]).max()) / float(np.abs(want["G"]).max())
    print(dict(d=d, J=J, functional=functional, rel_Hv=rel, rel_G=relG, dJ=abs(got["J"] - want["J"])))
    assert size >= 1e-3 and np.abs(want["G"]).max() >= 1e-3
    assert BUILTIN_HV_REL_MEASURED < 1e-13 and BUILTIN_G_REL_MEASURED < 1e-13
    assert rel <= 10 * BUILTIN_HV_REL_MEASURED and relG <= 10 * BUILTIN_G_REL_MEASURED
    assert abs(got["J"] - want["J"]) <= 1e-15


def _hs(pr, x, V, **kw):
    return osr.evaluate_chi(pr, x, V, osr.hilbert_schmidt(pr["target"], pr["weights"]), **kw)


@pytest.mark.parametrize("d", [3, 5])
def test_hilbert_schmidt_functional_against_central_differences(d):
    """H v against (4 D(h/2) - D(h)) / 3 with D(h) = (G(x + h v) - G(x - h v)) / (2 h) of the reference's own G, and G.v against
    the same differences of J; h = 4e-3: truncation O(h^4) ~ 1e-11 relative, rounding 1e-16 / h.  Measured 1.5e-12 (H v) and
    5.5e-11 (G.v, a cancelling sum of 2.4e-3) relative; asserted at ten times the larger."""
    pr = _case(d, 2)
    x = pr["pulsevals"]
    v = ohr.directions(77 + d, 1, x.size)[0]
    want = _hs(pr, x, v)
    osr.assert_reference_conditions(want)
    h = 4e-3
    at = {s: _hs(pr, x + s * h * v, v) for s in (-1.0, -0.5, 0.5, 1.0)}
    rich = lambda key: (4 * (at[0.5][key] - at[-0.5][key]) / h - (at[1.0][key] - at[-1.0][key]) / (2 * h)) / 3   # noqa: E731
    relH = float(np.abs(want["Hv"] - rich("G")).max()) / float(np.abs(want["Hv"]).max())
    Gv = float(want["G"] @ v)
    relG = abs(Gv - float(rich("J"))) / abs(Gv)
    print(dict(d=d, rel_Hv=relH, rel_Gv=relG, Gv=Gv))
    assert abs(Gv) >= 1e-3
    bound = 10 * max(FD_HV_REL_MEASURED, FD_G_REL_MEASURED)
    assert relH <= bound and relG <= bound


@pytest.mark.parametrize("d,J", [(4, 2), (17, 1)])
def test_double_against_long_double(d, J):
    """complex128 against clongdouble: at most 1 % of the bound of the shared comparison"""
    pr = _case(d, J, L=1, K=1, weights=False) if d > 8 else _case(d, J)
    x = pr["pulsevals"]
    v = ohr.directions(5 + d, 1, x.size)[0]
    a = _hs(pr, x, v)
    b = _hs(pr, x, v, dtype=np.clongdouble)
    osr.assert_reference_conditions(a)
    dev = float(np.abs(a["Hv"] - np.asarray(b["Hv"], dtype=float)).max())
    devG = float(np.abs(a["G"] - np.asarray(b["G"], dtype=float)).max())
    print(dict(d=d, dev_Hv=dev, dev_G=devG, bound=ohr.tol_hv(a["Hv"])))
    assert dev <= 0.01 * ohr.tol_hv(a["Hv"])
    assert devG <= 0.01 * ohr.tol_hv(a["G"])


def test_the_shared_comparison_refuses_wrong_boundaries():
    """each mutation deviates by at least 100 x the bound, and the comparison raises"""
    pr = _case(5, 2, hermitian=False, non_hermitian_states=0.3)
    x = pr["pulsevals"]
    V = ohr.directions(123, 2, x.size)
    hs = osr.hilbert_schmidt(pr["target"], pr["weights"])
    want = osr.evaluate_chi(pr, x, V, hs, want_parts=True)
    assert osr.assert_open_hvp_split_agrees(want["Hv"], want, "itself") == 0.0
    chi, dchi, S, SP = want["chi"], want["dchi"], want["S"], want["SP"]
    from_rho = hs(want["rhoT"], np.broadcast_to(want["rhoT"], want["drhoT"].shape))[2]
    wrong = {
        "chi' = 0": osr.contract(chi, np.zeros_like(dchi), S, SP)[1],
        "chi' from rho(T)": osr.contract(chi, from_rho, S, SP)[1],
        "rho' dropped in the overlaps": osr.evaluate_chi(pr, x, V, hs, wrong="drop_rho_prime")["Hv"],
        "dchi transposed": osr.contract(chi, np.swapaxes(dchi, -1, -2), S, SP)[1],
        "chi' conjugated": osr.contract(chi, np.conj(dchi), S, SP)[1],
    }
    tol = ohr.tol_hv(want["Hv"])
    for label, Hv in wrong.items():
        dev = float(np.abs(Hv - want["Hv"]).max())
        print(label, dict(dev=dev, times_tol=dev / tol))
        assert dev >= 100 * tol, label
        with pytest.raises(AssertionError):
            osr.assert_open_hvp_split_agrees(Hv, want, label)
    # and a reference whose chi' hardly matters is refused by the conditions, whatever is compared with it
    weak = dict(want, Hv_chi0=want["Hv"] * (1 - 1e-3))
    with pytest.raises(AssertionError):
        osr.assert_open_hvp_split_agrees(want["Hv"], weak, "chi' without weight")
