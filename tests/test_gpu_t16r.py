"""expm_t16r_asm on the device (needs an MI355X): the cells of expm_t16q_asm with the tile exchanges of the two Hermitian squares
sent under the last matrix instructions of the square (grape.jl_amd/csrc/asm/gen_t16r.py).  The arithmetic is unchanged, operation
for operation, so the yardstick is expm_t16q_asm itself: GRAPE_EXPM_T16Q=1 GRAPE_EXPM_T16R=1 against GRAPE_EXPM_T16Q=1
GRAPE_EXPM_T16R=0 on the same handle must give the same bits everywhere -- J, G, tau, the stored states, every propagator -- and the
same counts, except the executed matrix instructions: 624 per marked cell and wave instead of 625.  One more shape is large enough
for the rule of grape_create to choose the kernel with nothing set."""
import os
import re

import numpy as np
import pytest

import t16q_reference as Q
from test_gpu_t16q import SHAPES, assert_same_bits, environment, handle, problem, run

pytestmark = pytest.mark.gpu

assert SHAPES == [(64, 2, 9, 3), (49, 1, 5, 2), (57, 2, 11, 2)]       # (N, L, N_T, K): both squares, padded tiles, both walk directions


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


def test_first_contact_one_evaluation_of_the_smallest_shape(g):
    """the narrowest run of the new kernel: ten cells, one evaluation"""
    pr = problem(*SHAPES[1])
    r = run(g, pr, GRAPE_EXPM_T16R=1)
    assert r["work"]["t16r_kernel"] == 1 and r["work"]["t16q_cells"] == pr["K"] * pr["N_T"] and r["work"]["asm_kernel"] == 1
    assert np.isfinite(r["J"]) and np.isfinite(r["U"]).all()


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "N%d-L%d-NT%d-K%d" % s)
def case(request, g):
    pr = problem(*request.param)
    q = Q.expected_q(pr)
    assert q.all()                                             # every cell certifiable, with margin: no squarings, all marked
    return pr, q, run(g, pr, GRAPE_EXPM_T16R=1), run(g, pr, GRAPE_EXPM_T16R=0)


def test_same_bits_as_expm_t16q_asm(case):
    pr, q, on, off = case
    assert on["work"]["t16r_kernel"] == 1 and off["work"]["t16r_kernel"] == 0
    assert_same_bits(on, off)


def test_same_counts_and_624_matrix_instructions_per_marked_cell(case):
    pr, q, on, off = case
    for name in ("t16q_cells", "walk_steps", "t16_cells", "t18_cells", "asm_kernel", "t16_certified", "seg_certified", "deriv_orders",
                 "t18_squarings"):
        assert on["work"][name] == off["work"][name], name
    marked = on["work"]["t16q_cells"]
    assert marked == q.sum() and on["work"]["asm_kernel"] == 1
    assert on["work"]["t18_mfma_flop"] == 2048.0 * 4 * (624 * marked + 2 * on["work"]["walk_steps"])
    assert off["work"]["t18_mfma_flop"] == 2048.0 * 4 * (625 * marked + 2 * off["work"]["walk_steps"])


def test_a_forced_route_keeps_expm_t16q_asm_unless_asked(g):
    """GRAPE_EXPM_T16Q=1 alone (what the neighbouring tests set): the kernel and the count they pin"""
    pr = problem(*SHAPES[1])
    r = run(g, pr)
    assert r["work"]["t16r_kernel"] == 0 and r["work"]["t16q_cells"] == pr["K"] * pr["N_T"]
    assert r["work"]["t18_mfma_flop"] == 2048.0 * 4 * (625 * r["work"]["t16q_cells"] + 2 * r["work"]["walk_steps"])
    # and without the route there is nothing for the switch to choose
    r = run(g, pr, GRAPE_EXPM_T16Q=0, GRAPE_EXPM_T16R=1)
    assert r["work"]["t16r_kernel"] == 0 and r["work"]["t16q_cells"] == 0


def rule_shape():
    """N = 64, L = 2, K = 2 and the smallest N_T at which grape_create turns the route on by itself: every workgroup of the launch
    (one per compute unit, never more than cells) walks at least T16Q_MIN_WALK cells"""
    import torch
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "grape.jl_amd", "csrc", "grape_kernels.hip.h")).read()
    min_walk = int(re.search(r"#define\s+T16Q_MIN_WALK\s+(\d+)", src).group(1))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K = 2

    def on(N_T):
        ncell = K * N_T
        return ncell >= min_walk * max(1, min(cus, ncell))
    N_T = next(n for n in range(1, 1 << 20) if on(n))
    assert on(N_T) and not on(N_T - 1)
    return 64, 2, N_T, K


def plain(g, pr, **env):
    """one evaluation with GRAPE_EXPM_T16Q unset"""
    old = os.environ.pop("GRAPE_EXPM_T16Q", None)
    try:
        with environment(**env):
            with handle(g, pr) as h:
                J, G, tau = h.eval(pr["pulsevals"])
                return dict(J=J, G=G.copy(), tau=tau.copy(), fw=h.storage(0), bw=h.storage(1), work=h.work(),
                            U=np.stack([h.propagator(k, n) for k in range(h.K) for n in range(h.N_T)]))
    finally:
        if old is not None:
            os.environ["GRAPE_EXPM_T16Q"] = old


def test_the_rule_itself_chooses_the_kernel(g, ref):
    assert "GRAPE_EXPM_T16R" not in os.environ
    shape = rule_shape()
    pr = problem(*shape)
    on, off = plain(g, pr), plain(g, pr, GRAPE_EXPM_T16R=0)
    marked = on["work"]["t16q_cells"]
    assert on["work"]["t16r_kernel"] == 1 and off["work"]["t16r_kernel"] == 0 and marked > 0 and off["work"]["t16q_cells"] == marked
    assert on["work"]["asm_kernel"] == 1
    assert_same_bits(on, off)
    assert off["work"]["t18_mfma_flop"] - on["work"]["t18_mfma_flop"] == 2048.0 * 4 * marked
    # one time step fewer: below the rule, the base kernel
    below = plain(g, problem(shape[0], shape[1], shape[2] - 1, shape[3]))
    assert below["work"]["t16r_kernel"] == 0 and below["work"]["t16q_cells"] == 0 and below["work"]["asm_kernel"] == 1
    # the C oracle at the suite's bars (its Taylor gradient: the same derivative as the default method to rounding, and seconds
    # instead of a minute at this many time steps)
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                gradient_method=ref.TAYLOR)
    dJ, dtau, dG = abs(on["J"] - Jr), np.abs(on["tau"] - taur).max(), np.abs(on["G"] - Gr).max() / np.abs(Gr).max()
    print("against the oracle: |dJ| %.2e, |dtau| %.2e, |dG| / max|G| %.2e" % (dJ, dtau, dG))
    assert dJ <= 1e-12 and dtau <= 1e-12 and dG <= 1e-10
