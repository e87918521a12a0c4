"""The reference of the split H v tests (tests/hvp_split_reference.py) proved on the CPU: against the proven reference of the
built-in functionals (tests/hvp_reference.py), against Richardson-extrapolated central differences for a functional the
library does not know (an expectation value, no targets), and by the shared comparison refusing three deliberately wrong
references.  No GPU, nothing of the product path."""
import numpy as np
import pytest

import hvp_reference as hr
import hvp_split_reference as sr

# 1. Deviation of evaluate_chi (built-in functionals written as a boundary callback) from hr.evaluate, relative to
# ||Hv||_inf, measured over the six cases below: exactly 0 for J, G, tau and Hv (the two assemble the same blocks in the same
# order, so they give the same bits).  The bound is ten times the largest, never looser than 1e-12: here, equality.
SAME_MEASURED = 0.0
SAME_BOUND = min(10.0 * SAME_MEASURED, 1e-12)
# 2. Deviation of evaluate_chi with the expectation-value functional from the Richardson-extrapolated central differences
# (h = 1e-2 and h / 2) of its own G, relative to ||Hv||_inf, measured over the cases below: 9.3e-10 (N = 5), 1.8e-9 (N = 3);
# G against the same differences of J: 3.0e-11, 3.3e-11 of ||G||_inf.  Ten times the largest, never looser than 1e-6.
FD_MEASURED, FD_G_MEASURED = 1.8e-9, 3.3e-11
FD_BOUND, FD_G_BOUND = min(10.0 * FD_MEASURED, 1e-6), min(10.0 * FD_G_MEASURED, 1e-6)


def small_problem(N, seed_tag):
    """K = 2, weights, shape, non-uniform grid (the recipe of tests/test_hvp_reference.py)"""
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


@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("functional", [0, 1, 2])
def test_builtin_functionals_as_a_boundary_reproduce_the_proven_reference(N, functional):
    pr = small_problem(N, functional)
    V = hr.directions(100 * N + functional, 2, pr["L"] * pr["N_T"])
    want = hr.evaluate(pr, pr["pulsevals"], V, functional)
    hr.assert_order_one(want)
    got = sr.evaluate_chi(pr, pr["pulsevals"], V, sr.builtin_boundary(pr, functional))
    fig = dict(dJ=abs(got["J"] - want["J"]), dG=float(np.abs(got["G"] - want["G"]).max() / np.abs(want["G"]).max()),
               dHv=float(np.abs(got["Hv"] - want["Hv"]).max() / np.abs(want["Hv"]).max()),
               dtau=float(np.abs(got["tau"] - want["tau"]).max()), bound=SAME_BOUND)
    print(dict(N=N, functional=functional), fig)
    assert fig["dJ"] <= SAME_BOUND and fig["dG"] <= SAME_BOUND and fig["dHv"] <= SAME_BOUND and fig["dtau"] <= SAME_BOUND
    assert got["dpsiT"].shape == (2, pr["K"], N) and got["dtau"].shape == (2, pr["K"])


def expectation_case(N, seed):
    """N_T = 4, K = 2, pulses x 3, no targets; O_k = gue(subseed(seed, 900 + k))"""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, 4, 2, seed=seed)
    pr["pulsevals"] = 3.0 * pr["pulsevals"]
    pr["target"] = None
    pr["shape"] = None
    return pr, sr.expectation_boundary(sr.observables(seed, 2, N), pr["weights"])


@pytest.fixture(scope="module")
def expectation_cases():
    out = {}
    for N in (3, 5):
        pr, boundary = expectation_case(N, 4000 + N)
        V = hr.directions(300 + N, 2, pr["L"] * pr["N_T"])
        out[N] = (pr, boundary, V, sr.evaluate_chi(pr, pr["pulsevals"], V, boundary))
    return out


@pytest.mark.parametrize("N", [3, 5])
def test_expectation_value_functional_against_finite_differences(expectation_cases, N):
    pr, boundary, V, want = expectation_cases[N]
    sr.assert_signals(want)
    assert want["tau"] is None and want["dtau"] is None
    x = pr["pulsevals"]
    zero = np.zeros_like(x)

    def value(y):
        return sr.evaluate_chi(pr, y, zero, boundary)

    h = 1e-2
    # G against central differences of J (Richardson, h and h / 2), one coordinate direction at a time
    Gfd = np.empty_like(x)
    for i in range(len(x)):
        e = np.zeros_like(x)
        e[i] = 1.0
        d1 = (value(x + h * e)["J"] - value(x - h * e)["J"]) / (2 * h)
        d2 = (value(x + 0.5 * h * e)["J"] - value(x - 0.5 * h * e)["J"]) / h
        Gfd[i] = (4.0 * d2 - d1) / 3.0
    relG = float(np.abs(Gfd - want["G"]).max() / np.abs(want["G"]).max())
    worst = 0.0
    for j, v in enumerate(V):
        d1 = (value(x + h * v)["G"] - value(x - h * v)["G"]) / (2 * h)
        d2 = (value(x + 0.5 * h * v)["G"] - value(x - 0.5 * h * v)["G"]) / h
        fd = (4.0 * d2 - d1) / 3.0
        worst = max(worst, float(np.abs(fd - want["Hv"][j]).max() / np.abs(want["Hv"][j]).max()))
    print(dict(N=N, fd_deviation_rel=worst, bound=FD_BOUND, fd_G_rel=relG, bound_G=FD_G_BOUND))
    assert worst <= FD_BOUND
    assert relG <= FD_G_BOUND


@pytest.mark.parametrize("N", [17, 33])
def test_signals_of_the_expectation_value_functional_at_the_gpu_sizes(N):
    """the sizes of tests/test_gpu_hvp_split.py beyond the two above: ||G||_inf, ||Hv||_inf are O(0.1)"""
    pr, boundary = expectation_case(N, 4000 + N)
    want = sr.evaluate_chi(pr, pr["pulsevals"], hr.directions(300 + N, 1, pr["L"] * pr["N_T"]), boundary)
    sr.assert_signals(want)


@pytest.mark.parametrize("wrong", sr.WRONG)
def test_the_comparison_refuses_wrong_references(expectation_cases, wrong):
    """dchi = 0, dchi built from Psi(T) instead of Psi'(T), Psi' dropped in the overlaps: each moves H v by far more than the
    bound of assert_hvp_agrees"""
    pr, boundary, V, want = expectation_cases[5]
    bad = sr.evaluate_chi(pr, pr["pulsevals"], V, boundary, wrong=wrong)
    hr.assert_hvp_agrees(want["Hv"], want["Hv"], "right")
    assert np.array_equal(bad["G"], want["G"])
    with pytest.raises(AssertionError):
        hr.assert_hvp_agrees(bad["Hv"], want["Hv"], wrong)
