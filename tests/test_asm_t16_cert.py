"""The certified bit of the four-product assembly cell (grape.jl_amd/csrc/asm/gen_t16.py): a cell whose spectrum the plan of
the evaluation certified from the trace tables (splan bit 8) skips the sums, reductions, LDS round trip and store of the
in-cell spectral bound.  Executed by the emulator of gcn.py with the bit set and with it clear on the same inputs:
everything the kernel hands on must be bit-identical, the verdict word must be left alone, and the emulator's checks
(outstanding loads, barrier epochs, wait states) must pass on both paths."""
import numpy as np
import pytest

from test_asm_kernel import gcn, gen_t16, make_inputs, run_kernel

CERT = gen_t16.CERT_BIT


@pytest.fixture(scope="module")
def program():
    g, prog, text = gen_t16.generate()
    return g, prog, text


@pytest.fixture(scope="module")
def inputs():
    KC, N_T = 1, 2
    H0, Sn, dts, H0f, Sf = make_inputs(64, KC, N_T, seed=31)
    dts[:] = [0.6, 1.9]                      # cell 0: s = 0, cell 1: exponentiated as A / 2 and squared once
    rng = np.random.default_rng(9)
    psi0 = rng.normal(size=(KC, 64)) + 1j * rng.normal(size=(KC, 64))
    return KC, N_T, H0f, Sf, dts, psi0


def test_wait_states_of_both_paths(program):
    _, prog, _ = program
    assert gcn.check_hazards(prog) == 0
    # the certified path adds no matrix instruction to the list (it passes through the one of the bound)
    assert prog.count("mfma") == 120 + 3 * 192 + 3 + 192


@pytest.mark.parametrize("carried", [False, True])
def test_certified_cells_hand_on_the_same_bits(program, inputs, carried):
    """cells with s = 0 and s = 1, with and without a carried walk state (one workgroup: an ascending walk over both cells)"""
    _, prog, _ = program
    KC, N_T, H0f, Sf, dts, psi0 = inputs
    sq = np.array([0, 1], np.int32)
    kw = dict(fuse=3 if carried else 0, psi0=psi0, chiT=psi0, want_state=True)
    U0, v0, st0, fw0, bw0, pg0 = run_kernel(prog, H0f, Sf, dts, KC, N_T, 1, splan=sq, **kw)
    U1, v1, st1, fw1, bw1, pg1 = run_kernel(prog, H0f, Sf, dts, KC, N_T, 1, splan=sq | CERT, **kw)
    assert list(v0) == [0, 0]                # (both cells are inside the bound: the in-cell verdict agrees with the bit)
    assert list(v1) == [-1, -1]              # the certified cell does not write the verdict word
    assert not np.isnan(U0).any()
    assert np.array_equal(U0.view(np.uint64), U1.view(np.uint64))
    assert np.array_equal(fw0.view(np.uint64), fw1.view(np.uint64))
    assert np.array_equal(bw0.view(np.uint64), bw1.view(np.uint64))
    assert np.array_equal(pg0, pg1)
    assert list(pg0[0]) == ([2] if carried else [0])
    # executed matrix instructions: the same on both paths (what t16_post_kernel books per cell)
    steps = 2 if carried else 0
    assert st0["mfma"] == st1["mfma"] == 4 * (697 * 2 + 192 + 2 * steps)


def test_one_certified_cell_beside_an_uncertified_one(program, inputs):
    """the bit is per cell: cell 0 certified, cell 1 on the in-cell verdict (which fails: s = 0 planned at dt = 1.9), the walk
    ends where it ends without the bit"""
    _, prog, _ = program
    KC, N_T, H0f, Sf, dts, psi0 = inputs
    kw = dict(fuse=3, psi0=psi0, chiT=psi0, want_state=True)
    U0, v0, st0, fw0, bw0, pg0 = run_kernel(prog, H0f, Sf, dts, KC, N_T, 1, splan=[0, 0], **kw)
    U1, v1, st1, fw1, bw1, pg1 = run_kernel(prog, H0f, Sf, dts, KC, N_T, 1, splan=[CERT, 0], **kw)
    assert list(v0) == [0, 1] and list(v1) == [-1, 1]
    assert np.array_equal(U0.view(np.uint64), U1.view(np.uint64))
    assert np.array_equal(fw0.view(np.uint64), fw1.view(np.uint64))
    assert np.array_equal(pg0, pg1) and list(pg0[0]) == [1]
    assert st1["mfma"] == st0["mfma"]
