"""expm_t16r_asm (grape.jl_amd/csrc/asm/gen_t16r.py): expm_t16q_asm with the tile exchanges of its two Hermitian squares sent
before the square is complete, and without the matrix instruction whose result the marked path of expm_t16q_asm drops.

The arithmetic is expm_t16q_asm's, operation for operation, so the yardstick is that kernel itself: both instruction lists are
executed by the emulator of gcn.py on the same inputs and everything they write -- results, carried states, verdicts, progress
words -- must be equal to the bit.  The emulator's own checks (a register touched under an outstanding load, an LDS word shared
by two waves inside one barrier epoch, an LDS write left un-waited at a barrier) run on every instruction of both lists; the new
list writes the exchange areas while other waves still read the planes and reuses the areas of the first exchange for the
second, which is what those checks are for here.  Executed matrix instructions: 624 per marked cell and wave against 625."""
import os
import subprocess

import numpy as np
import pytest

from test_asm_kernel import gcn, make_inputs, run_kernel, t16_walks
from test_asm_t16q import Q, THETA_Q, radius, scaled_inputs

import gen_t16q  # noqa: E402  (test_asm_kernel put the generator directory on the path)
import gen_t16r  # noqa: E402


@pytest.fixture(scope="module")
def programs():
    return gen_t16r.generate(), gen_t16q.generate()


def both(programs, *args, **kw):
    """the two lists on the same inputs; every output bit for bit; returns (outputs of the new kernel, of expm_t16q_asm)"""
    (_, prog_r, _), (_, prog_q, _) = programs
    out_r, out_q = run_kernel(prog_r, *args, **kw), run_kernel(prog_q, *args, **kw)
    for a, b in zip(out_r, out_q):
        if isinstance(a, np.ndarray):       # (the bits, not the values: -0.0 against 0.0 must not pass, untouched NaN words must)
            bits = np.uint64 if a.dtype == np.complex128 else a.dtype
            assert np.array_equal(np.ascontiguousarray(a).view(bits), np.ascontiguousarray(b).view(bits))
    return out_r, out_q


def test_generated_program_has_no_missing_wait_states(programs):
    (_, prog, _), (_, prog_q, _) = programs
    assert gcn.check_hazards(prog) == 0
    # the list of expm_t16q_asm without the instruction that stands for the bound's on the marked path
    assert prog.count("mfma") == 120 + 3 * 192 + 3 + 192 + 120
    assert prog.count("mfma") == prog_q.count("mfma") - 1
    # the same vector and LDS instructions, the same barriers: only their places differ
    for kind in ("valu", "dpp", "lds", "vmem", "barrier", "smem"):
        assert prog.count(kind) == prog_q.count(kind), kind


def test_text_assembles_for_gfx950(programs, tmp_path):
    clang = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(clang):
        pytest.skip("no ROCm assembler")
    (_, _, text), _ = programs
    s = tmp_path / "k.s"
    s.write_text(text)
    subprocess.run([clang, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(s), "-o", str(tmp_path / "k.o")],
                   check=True)


@pytest.mark.parametrize("N,KC,N_T,nblk", [(64, 2, 5, 8), (57, 1, 3, 8), (49, 1, 3, 8)])
def test_marked_and_unmarked_cells_equal_the_twin(programs, N, KC, N_T, nblk):
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=N + KC, rho=0.99 * THETA_Q)
    cells = KC * N_T
    splan = np.array([Q if c % 3 != 1 else 0 for c in range(cells)], np.int32)
    q = int((splan != 0).sum())
    assert 0 < q < cells
    (U, verdict, stats), (_, _, stats_q) = both(programs, H0f, Sf, dts, KC, N_T, nblk, splan=splan)
    assert not np.isnan(U).any()
    # the verdict word of a marked cell is the plan's (the harness leaves -1 there); the others carry the in-cell bound's, which
    # is the twin's (compared above)
    assert np.array_equal(verdict[splan != 0], np.full(q, -1)) and np.isin(verdict[splan == 0], (0, 1)).all()
    assert stats["mfma"] == 4 * (624 * q + 697 * (cells - q)) and stats_q["mfma"] == stats["mfma"] + 4 * q


def test_walks_cross_from_marked_to_unmarked_cells_and_back(programs):
    """one ascending and one descending walk over three cells each, the middle one unmarked"""
    N, KC, N_T = 64, 1, 6
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=19, rho=0.97 * THETA_Q)
    splan = np.array([Q, 0, Q, Q, 0, Q], np.int32)
    rng = np.random.default_rng(6)
    psi0 = rng.normal(size=(KC, N)) + 1j * rng.normal(size=(KC, N))
    chiT = rng.normal(size=(KC, N)) + 1j * rng.normal(size=(KC, N))
    (U, verdict, stats, fw, bw, prog_), _ = both(programs, H0f, Sf, dts, KC, N_T, 2, fuse=3, psi0=psi0, chiT=chiT, want_state=True,
                                                 splan=splan)
    assert [tuple(r[:3]) for r in t16_walks(KC, N_T, 2)] == [(0, 3, 1), (5, 3, -1)]
    assert list(verdict) == [-1, 0, -1, -1, 0, -1]
    assert list(prog_[0]) == [3] and list(prog_[1]) == [3]
    assert not np.isnan(fw[0, 1:4]).any() and not np.isnan(bw[0, 3:6]).any()
    assert stats["mfma"] == 4 * (624 * 4 + 697 * 2 + 2 * 6)


def test_a_cell_with_a_planned_squaring_between_marked_cells(programs):
    N, KC, N_T = 64, 1, 3
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=23, rho=0.97 * THETA_Q)
    dts[1] *= 1.9 / radius(H0, Sn, dts, 0, 1)          # spectral radius 1.9: exponentiated as A / 2 and squared once
    splan = np.array([Q, 1, Q], np.int32)
    rng = np.random.default_rng(8)
    psi0 = rng.normal(size=(KC, N)) + 1j * rng.normal(size=(KC, N))
    (U, verdict, stats, fw, bw, prog_), _ = both(programs, H0f, Sf, dts, KC, N_T, 1, fuse=3, psi0=psi0, chiT=psi0, want_state=True,
                                                 splan=splan)
    assert list(verdict) == [-1, 0, -1] and list(prog_[0]) == [3]
    assert stats["mfma"] == 4 * (624 * 2 + 697 + 192 + 2 * 3)


@pytest.mark.parametrize("N,fuse", [(57, 1), (57, 2)])
def test_ascending_and_descending_walks_over_marked_cells(programs, N, fuse):
    """one workgroup per direction (fuse bit 0: the ascending walk propagates and stores transposed; bit 1: the descending one)"""
    KC, N_T = 1, 4
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=31 + fuse, rho=0.9 * THETA_Q)
    splan = np.full(N_T, Q, np.int32)
    rng = np.random.default_rng(fuse)
    psi0 = rng.normal(size=(KC, N)) + 1j * rng.normal(size=(KC, N))
    (U, verdict, stats, fw, bw, prog_), _ = both(programs, H0f, Sf, dts, KC, N_T, 2, fuse=fuse, psi0=psi0, chiT=psi0, want_state=True,
                                                 splan=splan)
    assert [tuple(r[:3]) for r in t16_walks(KC, N_T, 2)] == [(0, 2, 1), (3, 2, -1)]
    assert list(prog_[:, 0]) == [2 if fuse & 1 else 0, 2 if fuse & 2 else 0]
    carried = 2
    assert stats["mfma"] == 4 * (624 * N_T + 2 * carried)


@pytest.mark.parametrize("opts", [{"x1late": True}, {"x2late": True}, {"split2=0": True}, {"split2=12": True},
                                  {"bloc": True, "nolead": True, "noride0": True}],
                         ids=lambda o: "+".join(o))
def test_timing_variants_are_the_same_program_to_the_bit(programs, opts):
    """the code objects the per-edit timing swaps in (one exchange left where expm_t16q_asm has it; the barrier of the second
    exchange in front of or behind all of slot 0's matrix instructions; every LDS instruction where it was moved to, but in the open)"""
    _, prog, _ = gen_t16r.generate(opts=opts)
    assert gcn.check_hazards(prog) == 0
    N, KC, N_T = 49, 1, 2
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=3, rho=0.9 * THETA_Q)
    splan = np.array([Q, Q], np.int32)      # (two marked cells in a row: the second exchange, then the first, in the same areas)
    both(((None, prog, None), programs[1]), H0f, Sf, dts, KC, N_T, 1, splan=splan)
