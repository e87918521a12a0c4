"""expm_t16q_asm on the device (needs an MI355X): cells the plan certifies for the segment 1.11 run their second product as a
Hermitian square with the coefficient set T16Q_* (grape_get_work[21] counts them).  GRAPE_EXPM_T16Q=1 forces the route on
these small handles (by rule they would keep the base kernel: fewer than 8 cells per workgroup).  Which cells qualify is
established on the CPU from the eigenvalues first (tests/t16q_reference.py), with every cell at least 0.5 % from an edge that
decides.  Bars: the C oracle's for J, tau and G; 4e-15 on the propagators against the route switched off (two polynomials
of the same function, each within 2.2e-16 of it on the segment, plus the rounding of four products at N = 64: 2e-15 each
against expm in the emulator tests); the same bar against the compiled twin (GRAPE_EXPM_ASM=0: expm_t18_kernel<4, true, true, T16>
takes the same path on the same bit, a second implementation of the decision's consumer on the device)."""
import os

import numpy as np
import pytest

import t16_route_reference as R
import t16q_reference as Q

pytestmark = pytest.mark.gpu

SHAPES = [(64, 2, 9, 3), (49, 1, 5, 2), (57, 2, 11, 2)]       # (N, L, N_T, K)


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


class environment:
    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def handle(g, pr):
    return g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], shape=pr.get("shape"))


def run(g, pr, evals=1, **env):
    env.setdefault("GRAPE_EXPM_T16Q", 1)
    with environment(**env):
        with handle(g, pr) as h:
            out = []
            for _ in range(evals):
                J, G, tau = h.eval(pr["pulsevals"])
                out.append(dict(J=J, G=G.copy(), tau=tau.copy(), fw=h.storage(0), bw=h.storage(1), work=h.work(),
                                U=np.stack([h.propagator(k, n) for k in range(h.K) for n in range(h.N_T)])))
            return out[0] if evals == 1 else out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def assert_same_bits(a, b):
    assert a["J"] == b["J"]
    for name in ("G", "tau", "fw", "bw", "U"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name


def assert_oracle(ref, pr, r):
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                gradient_method=ref.GRADGEN)
    dJ, dtau, dG = abs(r["J"] - Jr), np.abs(r["tau"] - taur).max(), np.abs(r["G"] - Gr).max() / np.abs(Gr).max()
    print("against the oracle: |dJ| %.2e, |dtau| %.2e, |dG| / max|G| %.2e" % (dJ, dtau, dG))
    assert dJ <= 1e-12 and dtau <= 1e-12 and dG <= 1e-10


def problem(N, L, N_T, K):
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=1)
    pr["shape"] = None
    return pr


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "N%d-L%d-NT%d-K%d" % s)
def case(request, g):
    """the problem, what the CPU expects, and one run each with the route on and off -- shared by the tests below"""
    pr = problem(*request.param)
    q = Q.expected_q(pr)
    assert q.all()                                             # every cell certifiable, with margin
    return pr, q, run(g, pr), run(g, pr, GRAPE_EXPM_T16Q=0)


def test_marked_cells_are_counted_and_match_the_oracle(case, ref):
    pr, q, on, off = case
    assert on["work"]["t16q_cells"] == q.sum() and off["work"]["t16q_cells"] == 0
    assert on["work"]["asm_kernel"] == 1 and off["work"]["asm_kernel"] == 1
    assert_oracle(ref, pr, on)
    # 625 instead of 697 matrix instructions per marked cell and wave (2048 flop each), everything else as before
    assert off["work"]["t18_mfma_flop"] - on["work"]["t18_mfma_flop"] == 2048.0 * 4 * 72 * q.sum()
    for name in ("t16_cells", "t18_cells", "t16_certified", "seg_certified", "deriv_orders", "walk_steps", "t18_squarings"):
        assert on["work"][name] == off["work"][name], name


def test_propagators_against_the_route_switched_off(case):
    pr, q, on, off = case
    dU = np.abs(on["U"] - off["U"]).max()
    print("max |U(route on) - U(route off)| %.2e" % dU)
    assert 0.0 < dU < 4e-15


def test_against_the_compiled_twin(g, case):
    """GRAPE_EXPM_ASM=0 with the route on: the same marked cells, 624 matrix instructions per marked cell and wave (the assembly
    kernel: 625, and 2 per carried step), propagators within 4e-15; with the route off the twin keeps the base cell"""
    pr, q, on, off = case
    twin, twin_off = run(g, pr, GRAPE_EXPM_ASM=0), run(g, pr, GRAPE_EXPM_ASM=0, GRAPE_EXPM_T16Q=0)
    assert twin["work"]["asm_kernel"] == 0 and twin_off["work"]["asm_kernel"] == 0
    assert twin["work"]["t16q_cells"] == on["work"]["t16q_cells"] == q.sum() and twin_off["work"]["t16q_cells"] == 0
    dU = np.abs(on["U"] - twin["U"]).max()
    print("max |U(assembly) - U(twin)|, route on: %.2e" % dU)
    assert dU < 4e-15
    assert 0.0 < np.abs(twin["U"] - twin_off["U"]).max() < 4e-15
    assert np.abs(twin_off["U"] - off["U"]).max() < 4e-15                   # (the base cells: the bar of tests/test_gpu_asm.py)
    assert twin_off["work"]["t18_mfma_flop"] == 2048.0 * 4 * 696 * q.size
    assert twin["work"]["t18_mfma_flop"] == 2048.0 * 4 * 624 * q.sum()
    assert on["work"]["t18_mfma_flop"] == 2048.0 * 4 * (625 * q.sum() + 2 * on["work"]["walk_steps"])
    for name in ("t16_cells", "t18_cells"):
        assert twin["work"][name] == on["work"][name], name
    assert abs(twin["J"] - on["J"]) <= 1e-12 and np.abs(twin["tau"] - on["tau"]).max() <= 1e-12


@pytest.mark.parametrize("switch", ["GRAPE_EXPM_CERT", "GRAPE_DERIV_SEG", "GRAPE_DERIV_ECON"])
def test_the_route_does_not_depend_on_the_other_switches(g, case, switch):
    """J, tau, fw, bw and U are the same bits; G too under the two switches that do not choose the derivative series"""
    pr, q, on, _ = case
    other = run(g, pr, **{switch: 0})
    assert other["work"]["t16q_cells"] == q.sum()
    assert other["J"] == on["J"]
    for name in ("tau", "fw", "bw", "U") + (("G",) if switch == "GRAPE_EXPM_CERT" else ()):
        assert np.array_equal(bits(other[name]), bits(on[name])), name
    if switch != "GRAPE_EXPM_CERT":      # another series for the same derivative (tests/test_gpu_deriv_seg.py: 1e-13)
        assert np.abs(other["G"] - on["G"]).max() <= 1e-13 * max(np.abs(on["G"]).max(), 1e-3)


def test_repeatable_over_evaluations_and_a_graph_replay(g):
    pr = problem(*SHAPES[0])
    first, second, third, fourth = run(g, pr, evals=4)
    for other in (second, third, fourth):
        assert_same_bits(first, other)
        assert other["work"]["t16q_cells"] == first["work"]["t16q_cells"] == pr["K"] * pr["N_T"]


def test_cells_beyond_the_segment_beyond_the_range_and_with_squarings(g, ref):
    """the inputs of the edge tests (t16_route_reference.edge_problem): interior cells inside 1.11 (marked), cells between 1.11
    and 1.36 (the base path of the same kernel), cells beyond 1.36 (handed to the five-product launch) and cells with one and
    two planned squarings, side by side in every walk"""
    pr = R.edge_problem("base")
    q = Q.expected_q(pr)
    d11, d136 = Q.margins(pr)
    dec = R.decide(pr)
    sq = dec["sq"]
    between = (sq == 0) & (d11 > 0) & (d136 < 0)
    handed = np.array([[k == R.HANDED for k in row] for row in dec["kind"]])
    assert q.sum() >= 8 and between.sum() >= 8 and (handed & (sq == 0)).any() and (sq > 0).any()
    on, off = run(g, pr), run(g, pr, GRAPE_EXPM_T16Q=0)
    assert on["work"]["t16q_cells"] == q.sum()
    assert on["work"]["t18_cells"] - on["work"]["t16_cells"] == dec["counts"]["handed_over"] == off["work"]["t18_cells"] - off["work"]["t16_cells"]
    assert on["work"]["t16_cells"] == off["work"]["t16_cells"] == dec["counts"]["t16_cells"]
    assert_oracle(ref, pr, on)
    # cells that are not marked run the base path: the same bits as with the route off
    U_on, U_off = on["U"].reshape(q.shape + on["U"].shape[1:]), off["U"].reshape(q.shape + off["U"].shape[1:])
    assert np.array_equal(bits(U_on[~q]), bits(U_off[~q]))
    assert np.abs(U_on[q] - U_off[q]).max() < 4e-15
    # the compiled twin plans no squarings: on this input more than a quarter of the cells are then out of range and it does not
    # try the four-product route at all.  Without the s = 2 edges (variant "s01") it does: the same marked cells as the assembly
    # route on that input, propagators at the same bar
    twin = run(g, pr, GRAPE_EXPM_ASM=0)
    assert twin["work"]["t16q_cells"] == 0 and twin["work"]["t16_cells"] == 0 and twin["work"]["asm_kernel"] == 0
    pr2 = R.edge_problem("s01")
    q2 = Q.expected_q(pr2)
    assert q2.sum() >= 8 and not q2.all()
    on2, twin2 = run(g, pr2), run(g, pr2, GRAPE_EXPM_ASM=0)
    assert twin2["work"]["t16q_cells"] == on2["work"]["t16q_cells"] == q2.sum() and twin2["work"]["t16_cells"] > 0
    shp = q2.shape + on2["U"].shape[1:]
    assert np.abs(twin2["U"].reshape(shp)[q2] - on2["U"].reshape(shp)[q2]).max() < 4e-15


def test_a_handle_below_the_rule_keeps_the_base_kernel(g):
    """switch unset: 27 cells on one workgroup per cell -- nothing changes, bit for bit"""
    pr = problem(*SHAPES[0])
    old = os.environ.pop("GRAPE_EXPM_T16Q", None)
    try:
        with handle(g, pr) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            w = h.work()
            U = np.stack([h.propagator(k, n) for k in range(h.K) for n in range(h.N_T)])
    finally:
        if old is not None:
            os.environ["GRAPE_EXPM_T16Q"] = old
    off = run(g, pr, GRAPE_EXPM_T16Q=0)
    assert w["t16q_cells"] == 0 and w["asm_kernel"] == 1
    assert J == off["J"] and np.array_equal(bits(G), bits(off["G"])) and np.array_equal(bits(U), bits(off["U"]))
