"""The reference of the H v tests (tests/hvp_reference.py) proved on the CPU: against Richardson-extrapolated central
differences of the oracle's gradient, by its symmetry, against closed-form second derivatives of two-level problems, and by
the shared comparison refusing five deliberately wrong references.  No GPU, nothing of the product path."""
import numpy as np
import pytest

import hvp_reference as hr

# Deviation of the reference from the Richardson-extrapolated central differences of grape_oracle.evaluate_gradient
# (steps h and h / 2, h = 1e-2), relative to ||Hv||_inf, measured over the six cases below: 2.5e-12 .. 3.9e-10 (the largest at N = 5, ss; the h^4 term of
# the extrapolation and the rounding of the oracle's gradient divided by h).  The bound is ten times that, and never looser
# than 1e-6 (so that the proof stays meaningful whatever a later measurement says).
FD_MEASURED = 3.9e-10
FD_BOUND = min(10.0 * FD_MEASURED, 1e-6)


def small_problem(N, functional, seed_tag):
    from grape_jl_amd import synth
    L, N_T, K = 2, 4, 2
    pr = synth.make_problem(N, L, N_T, K, seed=synth.BASE_SEED ^ (7000 + 10 * N + seed_tag))
    u = synth.uniform01(synth.subseed(pr["N"] + 31 * seed_tag, 8100), N_T + L * N_T)
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(0.5 + u[:N_T])])
    pr["shape"] = 0.5 + 0.5 * u[N_T:].reshape(L, N_T)
    pr["weights"] = np.array([1.5, 0.5])
    pr["pulsevals"] = 3.0 * pr["pulsevals"]
    hr.order_one_targets(pr)
    return pr


@pytest.fixture(scope="module")
def cases():
    out = {}
    for N in (2, 5):
        for functional in (0, 1, 2):
            pr = small_problem(N, functional, functional)
            V = hr.directions(100 * N + functional, 2, pr["L"] * pr["N_T"])
            out[(N, functional)] = (pr, V, hr.evaluate(pr, pr["pulsevals"], V, functional))
    return out


@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("functional", [0, 1, 2])
def test_reference_against_finite_differences_of_the_oracle_gradient(cases, N, functional):
    import grape_oracle as go
    pr, V, want = cases[(N, functional)]
    hr.assert_order_one(want)
    x = pr["pulsevals"]

    def grad(y):
        return go.evaluate_gradient(pr["H0"], pr["Hc"], pr["tlist"], y, pr["psi0"], pr["target"], pr["weights"],
                                    functional=functional, shape=pr["shape"])[1]

    assert np.abs(grad(x) - want["G"]).max() <= 1e-12 * max(np.abs(want["G"]).max(), 1.0)
    h = 1e-2
    worst = 0.0
    for j, v in enumerate(V):
        d1 = (grad(x + h * v) - grad(x - h * v)) / (2 * h)
        d2 = (grad(x + 0.5 * h * v) - grad(x - 0.5 * h * v)) / h
        fd = (4.0 * d2 - d1) / 3.0
        rel = np.abs(fd - want["Hv"][j]).max() / np.abs(want["Hv"][j]).max()
        worst = max(worst, rel)
    print(dict(N=N, functional=functional, fd_deviation_rel=worst, bound=FD_BOUND))
    assert worst <= FD_BOUND


@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("functional", [0, 1, 2])
def test_reference_is_symmetric(cases, N, functional):
    _, V, want = cases[(N, functional)]
    a, b = float(V[0] @ want["Hv"][1]), float(V[1] @ want["Hv"][0])
    print(dict(vHw=a, wHv=b))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b), np.abs(want["Hv"]).max())


def test_closed_form_second_derivative_of_the_two_level_problems():
    """one control, one step of length T.  H = eps sigma_x, |0> -> |1>: J = cos^2(eps T), J'' = -2 T^2 cos(2 eps T).
    The README problem H = sigma_z + eps sigma_x: J = 1 - u q with u = eps^2 / W^2, q = sin^2(W T), W = sqrt(1 + eps^2) (Rabi)."""
    sz, sx = np.diag([1.0, -1.0]).astype(complex), np.array([[0, 1], [1, 0]], complex)
    base = dict(Hc=sx[None], psi0=np.array([[1, 0]], complex), target=np.array([[0, 1]], complex))
    e, T = 0.37, 1.3
    for functional in (0, 1):   # (one trajectory, weight 1: sm and ss are the same function)
        got = hr.evaluate(dict(base, H0=np.zeros((1, 2, 2), complex), tlist=np.array([0.0, T])), [e], [1.0], functional)
        assert abs(got["J"] - np.cos(e * T) ** 2) <= 1e-14
        assert abs(got["G"][0] + T * np.sin(2 * e * T)) <= 1e-13
        assert abs(got["Hv"][0] + 2 * T * T * np.cos(2 * e * T)) <= 1e-12
        W = np.sqrt(1 + e * e)
        u, u1, u2 = e * e / W ** 2, 2 * e / W ** 4, (2 - 6 * e * e) / W ** 6
        q = np.sin(W * T) ** 2
        q1 = np.sin(2 * W * T) * T * e / W
        q2 = 2 * np.cos(2 * W * T) * (T * e / W) ** 2 + np.sin(2 * W * T) * T / W ** 3
        got = hr.evaluate(dict(base, H0=sz[None], tlist=np.array([0.0, T])), [e], [1.0], functional)
        assert abs(got["J"] - (1 - u * q)) <= 1e-14
        assert abs(got["G"][0] + (u1 * q + u * q1)) <= 1e-13
        assert abs(got["Hv"][0] + (u2 * q + 2 * u1 * q1 + u * q2)) <= 1e-12
    # J_T_re on the same step: tau = -i (eps / W) sin(W T) is imaginary, so J = 1 and every derivative vanishes
    got = hr.evaluate(dict(base, H0=sz[None], tlist=np.array([0.0, T])), [e], [1.0], 2)
    assert abs(got["J"] - 1.0) <= 1e-14 and abs(got["Hv"][0]) <= 1e-12


@pytest.mark.parametrize("wrong", hr.WRONG)
def test_the_comparison_refuses_wrong_references(cases, wrong):
    """every deliberate mistake moves H v by far more than the bound of assert_hvp_agrees (functional sm: chi'(T) matters)"""
    pr, V, want = cases[(5, 0)]
    bad = hr.evaluate(pr, pr["pulsevals"], V, 0, wrong=wrong)
    hr.assert_hvp_agrees(want["Hv"], want["Hv"], "right")
    with pytest.raises(AssertionError):
        hr.assert_hvp_agrees(bad["Hv"], want["Hv"], wrong)
