"""Self-checks of tests/t16_route_reference.py (CPU): the inputs of tests/test_gpu_t16_edges.py reach the edges they are built
for, no cell of any input is undecidable, the reference propagators agree with scipy, the double-precision divided
differences with the C oracle, and the bar the GPU test holds the economized derivative series to discriminates."""
import os
import sys

import numpy as np
import pytest

import t16_route_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VARIANTS = ("base", "s01", "pertraj", "shape", "negative")
# counts of the reference per input: (certified, kept by the four-product route, handed over)
COUNTS = {"base": (53, 55, 17), "s01": (56, 58, 14), "pertraj": (53, 55, 17), "shape": (50, 52, 20), "negative": (53, 55, 17)}


@pytest.fixture(scope="module")
def problems():
    return {v: R.edge_problem(v) for v in VARIANTS}


@pytest.fixture(scope="module")
def decisions(problems):
    return {v: R.decide(pr) for v, pr in problems.items()}


def test_the_generator_has_one_outlier_eigenvalue_and_the_figures_the_edges_rest_on(problems):
    pr = problems["base"]
    m8, lam = R.m8_of(pr, R.KSTAR, 0)
    a = np.sort(np.abs(lam))
    print("rho = %.4f, next %.3f, m8^(1/8) / rho = %.6f" % (a[-1], a[-2], m8 ** 0.125 / a[-1]))
    assert 1.04 < a[-1] < 1.07 and a[-2] < 0.31                  # one outlier, the bulk is the weak drift
    assert 1.0 < m8 ** 0.125 / a[-1] < 1.00005                   # the Schatten-8 bound IS the spectral radius here
    ops, e = R.operators(pr, R.KSTAR), R.amplitudes(pr, 0)
    H = ops[0] + e[0] * ops[1] + e[1] * ops[2]
    for s in (0, 1, 2):
        dt = R.edge_dt(pr, R.KSTAR, 0, s, 0.0)
        r = R.plan_estimate(ops, e, dt)
        assert abs(r / 2 ** s - 1.0514) < 2e-3                   # the plan's estimate at the edge: inside 1.15 / 1.11 ...
        assert R.plan_squarings(r)[:2] == (s, False)             # ... so the edge of s squarings is planned with s squarings
        A2 = (H @ H) * (dt / 2 ** s) ** 2
        n2 = (np.abs(A2.real) + np.abs(A2.imag)).sum(axis=0).max() / R.THETA ** 2
        assert n2 > 2.0                                          # the 1-norm alternative fails with margin
    # a semicircle spectrum cannot reach the s >= 1 edges: at m8^(1/8) dt = 2 theta the plan's estimate is 2 theta / 3.5^(1/8),
    # which two squarings bring below 1.11 -- the plan over-squares it
    assert R.plan_squarings(2.0 * R.THETA / 3.5 ** 0.125)[0] == 2


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_edge_cell_is_what_it_was_built_to_be_and_no_cell_is_undecidable(problems, decisions, variant):
    pr, dec = problems[variant], decisions[variant]
    assert dec["counts"]["undecidable"] == 0 and not dec["skipped"] and dec["counts"]["out"] == 0
    for k in range(R.K):      # Hermitian to the last bit: anything else is a general generator to the handle (expm_t18g_asm)
        assert all(np.array_equal(O, O.conj().T) for O in R.operators(pr, k))
    for n, s, delta in pr["edge_steps"]:
        assert dec["sq"][R.KSTAR, n] == s
        assert abs(dec["delta"][R.KSTAR, n] - delta) <= 1e-12    # (rounding of the cumulative time grid: far inside every band)
        assert dec["kind"][R.KSTAR][n] == R.EXPECTED[delta], (n, s, delta)
    # the trajectory 3 % inside is certified throughout, the one 2.5 % beyond is handed over at every edge step
    edge = [n for n, _, _ in pr["edge_steps"]]
    assert all(dec["kind"][1][n] == R.CERTIFIED for n in range(R.N_T))
    assert all(dec["kind"][2][n] == (R.HANDED if n in edge else R.CERTIFIED) for n in range(R.N_T))
    c = dec["counts"]
    assert (c["certified"], c["t16_cells"], c["handed_over"]) == COUNTS[variant]
    # both derivative batches of the chosen trajectory hold edge cells; the economized series runs at both radii on the
    # trajectory inside, and not on a batch with a cell that was handed over or squared twice
    assert any(n < 16 for n in edge) and any(n >= 16 for n in edge)
    eb = R.econ_batches(dec)
    assert eb[1][0] == 2 * R.THETA and eb[R.KSTAR] == [0.0, 0.0] and eb[2] == [0.0, 0.0]
    assert eb[1][1] == (2 * R.THETA if variant == "s01" else 0.0)
    # without the certificate the same cells are kept, none certified
    off = R.decide(pr, cert=False)["counts"]
    assert off["certified"] == 0 and off["t16_cells"] == c["t16_cells"] and off["undecidable"] == 0


def test_the_shape_alone_carries_two_cells_across_the_edge(problems):
    pr = problems["shape"]
    dec, flat = R.decide(pr), R.decide(dict(pr, shape=None))
    for n, want in ((2, R.CERTIFIED), (19, R.HANDED)):
        assert dec["kind"][R.KSTAR][n] == want and flat["kind"][R.KSTAR][n] == R.CERTIFIED
        assert flat["delta"][R.KSTAR, n] < -0.9                  # without the shape: far inside


def test_negative_pulses_reach_the_odd_monomials(problems):
    pr = problems["negative"]
    t8, t6, ex8, ex6 = R.decide(pr)["tables"][0]
    e = R.amplitudes(pr, 0)
    odd = (ex8.sum(axis=1) % 2) == 1
    mono = np.prod(e[None, :] ** ex8, axis=1)
    assert np.all(e < 0) and np.abs(t8[odd] * mono[odd]).max() > 1e-3 * np.abs(t8 * mono).max()


def test_without_planned_squarings(problems):
    """GRAPE_EXPM_SQ=0: every cell beyond the plan's 1.15 is out of range; the 21 of the base input are more than a quarter of
    72 (the route is not tried), the 15 of the input without s = 2 edges are not (they are handed over one by one)"""
    d = R.decide(problems["base"], sq_on=False)
    assert d["counts"]["out"] == 21 and d["skipped"] and d["counts"]["t16_cells"] == 0 and d["counts"]["undecidable"] == 0
    d = R.decide(problems["s01"], sq_on=False)
    assert d["counts"]["out"] == 15 and not d["skipped"] and d["counts"]["undecidable"] == 0
    edge1 = [n for n, s, _ in problems["s01"]["edge_steps"] if s == 1]
    assert all(d["kind"][k][n] == R.HANDED for k in range(R.K) for n in edge1)
    assert (d["counts"]["certified"], d["counts"]["t16_cells"], d["counts"]["handed_over"]) == (49, 50, 22)


def test_quarter_rule_input():
    pr = R.quarter_problem()
    d = R.decide(pr)
    assert d["counts"]["out"] == 21 and 4 * d["counts"]["out"] > d["counts"]["ncell"] and d["skipped"]
    assert d["counts"]["undecidable"] == 0 and d["counts"]["t16_cells"] == 0
    # ... and the cells the plan certifies before the route is given up are there: 51 verdicts written for nothing
    assert sum(row.count(R.CERTIFIED) for row in d["kind"]) == 51


def test_stale_state_inputs():
    pr, A, B, grid2, X, Y = R.stale_problem()
    for x, tl, kx, ky in ((A, None, R.HANDED, R.CERTIFIED), (B, None, R.CERTIFIED, R.HANDED), (A, grid2, R.CERTIFIED, R.CERTIFIED)):
        d = R.decide(R.with_pulses(pr, x, tl))
        assert d["counts"]["undecidable"] == 0 and d["kind"][0][X] == kx and d["kind"][0][Y] == ky
        assert d["counts"]["handed_over"] == (kx == R.HANDED) + (ky == R.HANDED) and np.all(d["sq"] == 0)


@pytest.mark.parametrize("variant", ("base", "shape", "negative"))
def test_reference_propagators_against_scipy(problems, variant):
    from scipy.linalg import expm
    pr = problems[variant]
    U, _ = R.propagators(pr)
    dts = np.diff(pr["tlist"])
    worst = 0.0
    for k in range(R.K):
        ops = R.operators(pr, k)
        for n in range(R.N_T):
            e = R.amplitudes(pr, n)
            ref = expm(-1j * dts[n] * (ops[0] + e[0] * ops[1] + e[1] * ops[2]))
            err = np.abs(U[k, n] - ref).max() / max(1.0, dts[n])
            worst = max(worst, err)
            assert err <= 2e-14, (k, n, err)
    print("worst |U - expm| / max(1, dt): %.2e" % worst)


def test_divided_differences_in_double_against_the_c_oracle(problems, ref):
    pr = problems["base"]
    for functional in (0, 1, 2):
        want = R.evaluate_dk(pr, functional)
        J, G, tau, parts = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                        functional=functional, want_parts=True)
        assert abs(J - want["J"]) <= 1e-12 and np.abs(tau - want["tau"]).max() <= 1e-12
        assert np.abs(G - want["G"]).max() <= 1e-10 * max(np.abs(G).max(), 1e-3)
        assert np.abs(parts["tau_grads"] - want["tau_grads"]).max() <= 1e-12 and np.abs(parts["psiT"] - want["psiT"]).max() <= 1e-12


def test_the_pin_inputs_sit_where_the_pin_file_says():
    from conftest import load_mpmath_pin64
    import json
    pr, want = load_mpmath_pin64("edge64")
    z = json.load(open(os.path.join(ROOT, "tests", "golden", "mpmath_pin_edge64.json")))
    delta = np.array([[float(x) for x in row] for row in z["edge_delta"]])
    assert z["edge_squarings"] == [0, 1, 0, 0]
    assert abs(delta[1, 0] + 1e-5) < 1e-9 and abs(delta[1, 1] + 1e-5) < 1e-9 and abs(delta[1, 2] - 1e-3) < 1e-9 and delta[1, 3] < -0.5
    pr = dict(pr, shape=None)
    d = R.decide(pr)
    assert d["counts"]["undecidable"] == 0 and np.abs(d["delta"] - delta).max() < 1e-12
    assert np.array_equal(d["sq"][0], z["edge_squarings"]) and np.array_equal(d["sq"][1], z["edge_squarings"])
    assert d["kind"][1] == [R.CERTIFIED, R.CERTIFIED, R.HANDED, R.CERTIFIED]
    # trajectory 0 is 0.6 % inside: every cell certified, so its batch gets the economized series of the 2.72 segment with
    # cells at 0.994 of both segment ends
    assert d["kind"][0] == [R.CERTIFIED] * 4 and np.all(d["delta"][0, :3] > -0.06) and R.econ_batches(d) == [[2 * R.THETA], [0.0]]
    # the reference evaluation in double against the 50-digit one
    for functional in (0, 1, 2):
        got, w = R.evaluate_dk(pr, functional), want[functional]
        assert abs(got["J"] - w["J"]) <= 1e-13 and np.abs(got["tau_grads"] - w["tau_grads"]).max() <= 2e-13 * np.abs(w["tau_grads"]).max()


def test_the_bar_of_the_economized_series_discriminates():
    """The GPU test lets the error of tau_grads under the economized series exceed the Taylor twin's (floored at one ulp of the
    scale) by a factor 4.  On the two-pass arithmetic in numpy, at the ends of both segments: the committed scalars pass that
    bar, Taylor coefficients of the same degree miss it by two orders of magnitude or more.  The set of ONE DEGREE LESS does
    NOT miss it: its truncation error (at most 1.3e-15 at the very end of the segment, weighted down by the contraction) stays
    below 4 ulp -- measured 1.8e-16 .. 3.4e-16 of ||E|| at 1.36 and 2.8e-17 .. 8.4e-17 at 2.72 against a bar of 8.9e-16.  A bar at
    the rounding level cannot tell it from the committed set; that is the job of tests/test_econ_coeffs.py, which holds the
    polynomial itself to 2.5e-16 on the segment and shows that one degree less exceeds it."""
    import econ_coeffs as ec
    from test_asm_deriv3 import econ_tables
    tabs = econ_tables()
    ulp = 2.0 ** -52
    for deg, th in ((16, 1.36), (21, 2.72)):
        theta = ec.mp.mpf(str(th))
        assert tabs[deg][0] == th
        committed = [(float(a), float(b)) for a, b in tabs[deg][1]]
        less = [(float(a), float(b)) for a, b in ec.table(ec.polynomial(theta, deg - 1))]
        taylor = [(1.0 / (a + 1), 1.0 / (a + 1)) for a in range(deg)]
        twin = [(1.0 / (a + 1), 1.0 / (a + 1)) for a in range(ec.taylor_degree(theta) + 2)]        # the converged Taylor sum
        for seed in range(3):
            bar = 4.0 * max(ec.check(twin, th, seed=seed, n=8), ulp)
            e_c, e_l, e_t = (ec.check(t, th, seed=seed, n=8) for t in (committed, less, taylor))
            print("degree %d, radius %.2f, seed %d: committed %.2e, one degree less %.2e, Taylor of the degree %.2e, bar %.2e"
                  % (deg, th, seed, e_c, e_l, e_t, bar))
            assert e_c <= bar
            assert e_t > 50.0 * bar
