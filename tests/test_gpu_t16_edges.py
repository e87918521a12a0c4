"""The four-product route at the edges of its certified range, on the device (needs an MI355X).  tests/t16_route_reference.py
restates the decisions -- the plan, the certificate, the cell's own test -- and builds inputs whose cells sit a relative 1e-3 ..
1e-7 inside and outside theta = 1.36 and, under one and two planned squarings, 2 theta and 4 theta; no cell of any input is within
the guard bands in which the device's rounding could decide either way (asserted on the CPU, tests/test_t16_route_reference.py).
Here: the counters equal the reference's counts, certificate on and off give the same bits, every propagator is at the
project's propagator bar against V exp(-i lam dt) V^dagger, J / tau / G / tau_grads at the bars of the golden fixtures against
the C oracle and at the bar of the absolute pins against a 50-digit evaluation (tests/golden/mpmath_pin_edge64.json); the
trace tables beyond one pass of the build, at L = 4 and at N < 64; the "more than a quarter out of range" exit."""
import functools
import os

import numpy as np
import pytest

import t16_route_reference as R
from test_cert_table import evaluate, trace_tables
from test_gpu_t16_cert import assert_same_bits, bits

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


class environment:
    """set, create the handle and use it, restore"""

    def __init__(self, cert=True, **env):
        self.env = dict(GRAPE_EXPM_CERT="1" if cert else "0", **env)

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def handle(g, pr, functional=0):
    return g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], shape=pr.get("shape"), functional=functional)


def collect(h, x, cells=None):
    J, G, tau = h.eval(x)
    K, N_T = h.K, h.N_T
    cells = [(k, n) for k in range(K) for n in range(N_T)] if cells is None else cells
    return dict(J=J, G=G.copy(), tau=tau.copy(), U=np.stack([h.propagator(k, n) for k, n in cells]), fw=h.storage(0), bw=h.storage(1),
                work=h.work(), tg=h.tau_grads())


def run(g, pr, cert=True, functional=0, **env):
    with environment(cert, **env):
        with handle(g, pr, functional) as h:
            return collect(h, pr["pulsevals"])


def handed_over(r):
    return r["work"]["t18_cells"] - r["work"]["t16_cells"]


def assert_counts(res, counts, certified):
    w = res["work"]
    print("t16_certified %d, t16_cells %d, handed over %d, t18_squarings %d (the reference: %s)"
          % (w["t16_certified"], w["t16_cells"], handed_over(res), w["t18_squarings"], counts))
    assert w["t16_certified"] == (counts["certified"] if certified else 0)
    assert w["t16_cells"] == counts["t16_cells"] and handed_over(res) == counts["handed_over"]
    # (the counter also books what the five-product launch squares in the cells handed over to it: a lower bound)
    assert w["t18_squarings"] >= counts["squarings_kept"]


@functools.lru_cache(maxsize=None)
def reference_propagators(name):
    pr = problem(name)
    return R.propagators(pr)[0]


@functools.lru_cache(maxsize=None)
def problem(name):
    return R.quarter_problem() if name == "quarter" else R.edge_problem(name)


def assert_propagators(U, Uref, dts):
    """the project's propagator bar (test_expm_kernel_vs_scipy): 2e-14 max(1, dt), unitarity 1e-13 max(1, dt)"""
    K, N_T, N = Uref.shape[:3]
    U = U.reshape(K, N_T, N, N)
    worst = worst_u = 0.0
    for k in range(K):
        for n in range(N_T):
            sc = max(1.0, dts[n])
            err, uni = np.abs(U[k, n] - Uref[k, n]).max() / sc, np.abs(U[k, n].conj().T @ U[k, n] - np.eye(N)).max() / sc
            worst, worst_u = max(worst, err), max(worst_u, uni)
            assert err <= 2e-14 and uni <= 1e-13, (k, n, err, uni)
    print("propagators: worst |U - Uref| / max(1, dt) %.2e, |U^dagger U - 1| / max(1, dt) %.2e" % (worst, worst_u))


def oracle(ref, pr, functional=0):
    """the C oracle; a shape function is folded into the amplitudes (d / d eps = S d / d (eps S))"""
    N_T = len(pr["tlist"]) - 1
    L = pr["pulsevals"].size // N_T
    S = np.ones((L, N_T)) if pr.get("shape") is None else np.asarray(pr["shape"]).reshape(L, N_T)
    J, G, tau, parts = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"] * S.reshape(-1), pr["psi0"], pr["target"],
                                    pr["weights"], functional=functional, want_parts=True)
    return dict(J=J, G=G * S.reshape(-1), tau=tau, tg=parts["tau_grads"] * S[None], psiT=parts["psiT"])


def assert_against_oracle(res, want):
    """the bars of the golden fixtures (tests/test_gpu_parity.py)"""
    eJ, et = abs(res["J"] - want["J"]), np.abs(res["tau"] - want["tau"]).max()
    eG, etg = np.abs(res["G"] - want["G"]).max() / max(np.abs(want["G"]).max(), 1e-3), np.abs(res["tg"] - want["tg"]).max()
    print("against the C oracle: J %.2e, tau %.2e, G %.2e (relative), tau_grads %.2e" % (eJ, et, eG, etg))
    assert eJ <= 1e-12 and et <= 1e-12 and eG <= 1e-10 and etg <= 1e-12
    assert np.abs(res["fw"][:, -1] - want["psiT"]).max() <= 1e-12


# ---------------------------------------------------------------- decisions and values at the edges
@pytest.mark.parametrize("variant", ("base", "s01", "pertraj", "shape", "negative"))
def test_cells_at_the_edges_take_the_route_the_reference_names(g, ref, variant):
    pr = problem(variant)
    dec = R.decide(pr)
    assert dec["counts"]["undecidable"] == 0
    on, off = run(g, pr, True), run(g, pr, False)
    assert on["work"]["asm_kernel"] == (3 if variant == "pertraj" else 1)
    assert_counts(on, dec["counts"], True)
    assert_counts(off, dec["counts"], False)
    assert_same_bits(on, off)
    assert np.array_equal(bits(on["tg"]), bits(off["tg"]))
    assert_propagators(on["U"], reference_propagators(variant), np.diff(pr["tlist"]))
    assert_against_oracle(on, oracle(ref, pr))
    # the double-precision divided differences of the reference module, cell by cell
    dk = R.evaluate_dk(pr)
    assert np.abs(on["tg"] - dk["tau_grads"]).max() <= 1e-12 and abs(on["J"] - dk["J"]) <= 1e-12


@pytest.mark.parametrize("variant", ("base", "s01"))
def test_without_planned_squarings_the_long_steps_go_to_the_five_product_launch(g, variant):
    """GRAPE_EXPM_SQ=0: the plan words carry the certified bit only and every cell beyond the plan's 1.15 counts as out of range --
    more than a quarter of the base input (the route is not tried), 15 of 72 cells without the s = 2 edges (handed over singly)"""
    pr = problem(variant)
    dec = R.decide(pr, sq_on=False)
    assert dec["counts"]["undecidable"] == 0 and dec["skipped"] == (variant == "base")
    on, off = run(g, pr, True, GRAPE_EXPM_SQ="0"), run(g, pr, False, GRAPE_EXPM_SQ="0")
    assert_counts(on, dec["counts"], True)
    assert_counts(off, dec["counts"], False)
    assert_same_bits(on, off)
    assert_propagators(on["U"], reference_propagators(variant), np.diff(pr["tlist"]))


# ---------------------------------------------------------------- the absolute pin at the edge
def pin_errors(res, w):
    sJ, sG, sT = max(1.0, abs(w["J"])), np.abs(w["G"]).max(), max(1.0, np.abs(w["tau"]).max())
    return dict(J=abs(res["J"] - w["J"]) / sJ, tau=np.abs(res["tau"] - w["tau"]).max() / sT, G=np.abs(res["G"] - w["G"]).max() / sG,
                psiT=np.abs(res["fw"][:, -1] - w["psiT"]).max() / sT, tg=np.abs(res["tg"] - w["tau_grads"]).max() / np.abs(w["tau_grads"]).max())


@pytest.mark.parametrize("functional", [0, 1, 2])
def test_absolute_pin_at_the_edges_and_the_economized_series_against_its_taylor_twin(g, functional):
    """tests/golden/mpmath_pin_edge64.json: trajectory 1 at delta = -1e-5 (s = 0), -1e-5 (s = 1), +1e-3 (s = 0, handed over);
    trajectory 0 is 0.6 % inside, all certified, so its derivative batch runs the economized series of the 2.72 segment with
    cells at 0.994 of the ends of both segments.  Bars of tests/test_gpu_reference_pins.py.  The error of tau_grads under the
    economized series may exceed the Taylor twin's (GRAPE_DERIV_ECON=0), floored at one ulp of the scale, by a factor 4 (the
    order of summation differs).  Measured on an MI355X: see DESIGN.md, "Reference tests at the edges of the four-product range"."""
    from conftest import load_mpmath_pin64
    pr, want = load_mpmath_pin64("edge64")
    pr = dict(pr, shape=None)
    dec = R.decide(pr)
    assert dec["counts"]["undecidable"] == 0 and R.econ_batches(dec) == [[2 * R.THETA], [0.0]]
    w = want[functional]
    econ = run(g, pr, True, functional, GRAPE_DERIV_ECON="1")
    twin = run(g, pr, True, functional, GRAPE_DERIV_ECON="0")
    assert econ["work"]["asm_kernel"] == 1 and econ["work"]["asm_deriv_kernel"] == 1
    assert_counts(econ, dec["counts"], True)
    e, t = pin_errors(econ, w), pin_errors(twin, w)
    print("functional %d against the 50-digit pin, economized series: %s" % (functional, {k: "%.2e" % v for k, v in e.items()}))
    print("functional %d against the 50-digit pin, Taylor twin:       %s" % (functional, {k: "%.2e" % v for k, v in t.items()}))
    print("series orders summed: economized %d, Taylor %d" % (econ["work"]["deriv_orders"], twin["work"]["deriv_orders"]))
    for r in (e, t):
        assert r["J"] <= 1e-13 and r["tau"] <= 1e-13 and r["psiT"] <= 1e-13 and r["G"] <= 2e-13 and r["tg"] <= 2e-13, r
    # the economized series ran (at 0.994 * 2.72 the Taylor sum needs more than its 21 terms), on the same propagators
    assert econ["work"]["deriv_orders"] < twin["work"]["deriv_orders"]
    assert econ["J"] == twin["J"] and np.array_equal(bits(econ["U"]), bits(twin["U"]))
    # per trajectory, so that the batch of the economized series is not hidden behind the other
    scale = np.abs(w["tau_grads"]).max()
    for k in range(2):
        ee, tt = np.abs(econ["tg"][k] - w["tau_grads"][k]).max(), np.abs(twin["tg"][k] - w["tau_grads"][k]).max()
        print("trajectory %d: tau_grads error economized %.2e, Taylor %.2e (scale %.2e)" % (k, ee, tt, scale))
        assert ee <= 4.0 * max(tt, 2.0 ** -52 * scale), (k, ee, tt)


# ---------------------------------------------------------------- tables beyond three classes
@pytest.mark.parametrize("case", ("a", "b", "c", "d", "e"))
def test_tables_built_in_several_passes_at_four_controls_and_below_64(g, case):
    pr = R.table_problem(case)
    K, N_T = pr["H0"].shape[0], 2
    L = pr["Hc"].shape[0]
    dec = R.decide(pr)
    cls, reps = dec["cls"], dec["reps"]
    with environment(True):
        with handle(g, pr) as h:
            h.eval(pr["pulsevals"], gradient=False)
            t8, t6, ex = h.cert_table()
            work = h.work()
    n8 = {2: 45, 3: 165, 4: 495}[L]
    n6 = {2: 28, 3: 84, 4: 210}[L]
    assert t8.shape == (len(reps), n8) and t6.shape == (len(reps), n6) and ex.shape == (n8 + n6, L)
    assert len(reps) == (2 if case == "e" else K)
    worst = worst_c = 0.0
    rng = np.random.default_rng(ord(case))
    for kc, k in enumerate(reps):
        ops = R.operators(pr, k)
        c8, c6, ex8, ex6 = dec["tables"][kc]
        assert np.array_equal(ex[:n8], ex8) and np.array_equal(ex[n8:], ex6)
        # coefficient by coefficient against the numpy restatement, relative to the largest of the class
        d8, d6 = np.abs(t8[kc] - c8).max() / np.abs(c8).max(), np.abs(t6[kc] - c6).max() / np.abs(c6).max()
        worst_c = max(worst_c, d8, d6)
        assert d8 <= 1e-12 and d6 <= 1e-12, (kc, d8, d6)
        samples = [R.amplitudes(pr, n) for n in range(N_T)] + [3.0 * (2.0 * rng.random(L) - 1.0), np.full(L, -3.0)]
        for e in samples:
            lam = np.linalg.eigvalsh(ops[0] + sum(e[l] * ops[1 + l] for l in range(L)))
            m8, m6 = np.sum(lam ** 8), np.sum(lam ** 6)
            p8, S8 = evaluate(t8[kc], ex[:n8], e)
            p6, _ = evaluate(t6[kc], ex[n8:], e)
            assert abs(p8 - m8) <= 1e-12 * m8 and abs(p6 - m6) <= 1e-12 * m6, (kc, p8 / m8 - 1, p6 / m6 - 1)
            assert abs(p8 - m8) <= 2.0 ** -30 * S8
            worst = max(worst, abs(p8 / m8 - 1), abs(p6 / m6 - 1))
    print("case %s: device tables against the numpy tables %.2e (of the largest coefficient), against the moments %.2e" % (case, worst_c, worst))
    # the cells of the CLASSES are what the plan certifies and the counter counts
    assert dec["counts"]["undecidable"] == 0 and work["t16_certified"] == dec["counts"]["certified"] == len(reps) * N_T
    assert work["t16_cells"] == dec["counts"]["t16_cells"]


def test_five_controls_have_no_tables_and_the_cells_decide_themselves(g, ref):
    from grape_jl_amd import synth
    pr = synth.make_problem(64, 5, 3, 2, seed=705)
    pr["shape"] = None
    dec = R.decide(pr)
    assert dec["tables"] == [None, None] and dec["counts"]["undecidable"] == 0
    with environment(True):
        with handle(g, pr) as h:
            res = collect(h, pr["pulsevals"])
            assert h.cert_table()[0].size == 0
    assert_counts(res, dec["counts"], True)
    assert res["work"]["t16_certified"] == 0
    assert_against_oracle(res, oracle(ref, pr))


# ---------------------------------------------------------------- more than a quarter out of range
def test_a_quarter_of_the_cells_out_of_range_on_a_handle_with_certified_cells(g, ref):
    """7 of 24 steps beyond 2^3 x range: the four-product kernels leave at once although the plan has certified (and written
    verdict 0 for) the other 51 cells; the five-product launch computes every cell and the derivative series must not read
    those verdicts"""
    pr = problem("quarter")
    dec = R.decide(pr)
    assert dec["skipped"] and 4 * dec["counts"]["out"] > dec["counts"]["ncell"] and dec["counts"]["undecidable"] == 0
    on, off = run(g, pr, True), run(g, pr, False)
    assert on["work"]["t16_cells"] == 0 and off["work"]["t16_cells"] == 0
    assert_counts(on, dec["counts"], True)
    assert_counts(off, dec["counts"], False)
    assert_same_bits(on, off)
    assert np.array_equal(bits(on["tg"]), bits(off["tg"]))
    assert_propagators(on["U"], reference_propagators("quarter"), np.diff(pr["tlist"]))
    assert_against_oracle(on, oracle(ref, pr))
