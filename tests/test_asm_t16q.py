"""expm_t16q_asm (grape.jl_amd/csrc/asm/gen_t16q.py): the four-product cell whose second product is a Hermitian square
(coefficient set T16Q_*, c2 = 0) on the cells the plan marks with splan bit 9, and the base cell on all others -- one kernel, one
scalar branch per cell.  Executed by the emulator of gcn.py against scipy's expm: marked and unmarked cells side by side,
walks that cross from one kind to the other and back, a cell with a planned squaring between marked ones, the executed
matrix instructions (625 per marked cell and wave against 697), the emulator's own checks (outstanding loads, barrier epochs,
wait states) on both paths -- and that the base generator still emits the program it emitted before this variant existed."""
import hashlib
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

from test_asm_kernel import gcn, gen_t16, make_inputs, run_kernel, t16_walks

import gen_t16q  # noqa: E402  (test_asm_kernel put the generator directory on the path)

Q = gen_t16q.Q_BIT
THETA_Q = 1.11
# sha256 of the text gen_t16.generate() emitted on the commit before this variant (computed from a checkout of it)
BASE_SHA256 = "2d11b2b45fb7e862579aba3f8c700e255cc6f5398d1833f86386594656027631"
BASE_P_SHA256 = "ce9009f3b9fbf4ae473d53244e98a70a37dd5fef58ea67d5be60735145571696"      # gen_t16p.generate(), likewise


@pytest.fixture(scope="module")
def program():
    g, prog, text = gen_t16q.generate()
    return g, prog, text


def radius(H0, Sn, dts, kc, n):
    return np.abs(np.linalg.eigvalsh(dts[n] * (H0[kc] + Sn[n]))).max()


def scaled_inputs(N, KC, N_T, seed, rho=1.0):
    """inputs whose largest cell has spectral radius rho"""
    H0, Sn, dts, H0f, Sf = make_inputs(N, KC, N_T, seed=seed)
    dts *= rho / max(radius(H0, Sn, dts, kc, n) for kc in range(KC) for n in range(N_T))
    return H0, Sn, dts, H0f, Sf


def test_base_generators_emit_what_they_emitted():
    assert "GRAPE_T16_OPTS" not in os.environ
    _, _, text = gen_t16.generate()
    assert hashlib.sha256(text.encode()).hexdigest() == BASE_SHA256
    import gen_t16p
    _, _, text = gen_t16p.generate()
    assert hashlib.sha256(text.encode()).hexdigest() == BASE_P_SHA256


def test_generated_program_has_no_missing_wait_states(program):
    _, prog, _ = program
    assert gcn.check_hazards(prog) == 0
    # the base list plus the second path: 120 of the square and the one instruction that stands for the bound's
    assert prog.count("mfma") == 120 + 3 * 192 + 3 + 192 + 120 + 1


def test_text_assembles_for_gfx950(program, tmp_path):
    clang = "/opt/rocm/lib/llvm/bin/clang"
    if not os.path.exists(clang):
        pytest.skip("no ROCm assembler")
    _, _, text = program
    s = tmp_path / "k.s"
    s.write_text(text)
    subprocess.run([clang, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(s), "-o", str(tmp_path / "k.o")],
                   check=True)


@pytest.mark.parametrize("N,KC,N_T,nblk", [(64, 2, 5, 8), (50, 1, 3, 8)])
def test_marked_and_unmarked_cells_match_expm(program, N, KC, N_T, nblk):
    _, prog, _ = program
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=N + KC, rho=0.99 * THETA_Q)
    cells = KC * N_T
    splan = np.array([Q if c % 3 != 1 else 0 for c in range(cells)], np.int32)
    q = int((splan != 0).sum())
    assert 0 < q < cells
    U, verdict, stats = run_kernel(prog, H0f, Sf, dts, KC, N_T, nblk, splan=splan)
    for kc in range(KC):
        for n in range(N_T):
            ref = scipy.linalg.expm(-1j * dts[n] * (H0[kc] + Sn[n]))
            err = np.abs(U[kc * N_T + n] - ref).max()
            assert err < 2e-15, (kc, n, err)
    # the verdict word of a marked cell is the plan's (the harness leaves -1 there); the others pass the in-cell bound
    assert np.array_equal(verdict, np.where(splan != 0, -1, 0))
    assert stats["mfma"] == 4 * (625 * q + 697 * (cells - q))
    # all cells unmarked: this kernel is the base kernel
    U0, v0, st0 = run_kernel(prog, H0f, Sf, dts, KC, N_T, nblk)
    Ub, vb, stb = run_kernel(gen_t16.generate()[1], H0f, Sf, dts, KC, N_T, nblk)
    assert np.array_equal(U0.view(np.uint64), Ub.view(np.uint64)) and np.array_equal(v0, vb) and st0["mfma"] == stb["mfma"]
    unmarked = splan == 0
    assert np.array_equal(U[unmarked].view(np.uint64), Ub[unmarked].view(np.uint64))


def test_walks_cross_from_marked_to_unmarked_cells_and_back(program):
    """one ascending and one descending walk over three cells each, the middle one unmarked: the state a walk carries rides on
    both kinds of results"""
    _, prog, _ = program
    N, KC, N_T = 64, 1, 6
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=19, rho=0.97 * THETA_Q)
    splan = np.array([Q, 0, Q, Q, 0, Q], np.int32)
    rng = np.random.default_rng(6)
    psi0 = rng.normal(size=(KC, N)) + 1j * rng.normal(size=(KC, N))
    chiT = rng.normal(size=(KC, N)) + 1j * rng.normal(size=(KC, N))
    U, verdict, stats, fw, bw, prog_ = run_kernel(prog, H0f, Sf, dts, KC, N_T, 2, fuse=3, psi0=psi0, chiT=chiT, want_state=True,
                                                  splan=splan)
    assert [tuple(r[:3]) for r in t16_walks(KC, N_T, 2)] == [(0, 3, 1), (5, 3, -1)]
    assert list(verdict) == [-1, 0, -1, -1, 0, -1]
    assert list(prog_[0]) == [3] and list(prog_[1]) == [3]
    Uref = np.stack([scipy.linalg.expm(-1j * dts[n] * (H0[0] + Sn[n])) for n in range(N_T)])
    assert np.abs(U - Uref).max() < 2e-15
    x = psi0[0]
    for n in range(3):
        x = Uref[n] @ x
        assert np.abs(fw[0, n + 1] - x).max() < 5e-15 * max(1.0, np.abs(x).max()), n
    y = chiT[0]
    for n in (5, 4, 3):
        y = Uref[n].conj().T @ y
        assert np.abs(bw[0, n] - y).max() < 5e-15 * max(1.0, np.abs(y).max()), n
    assert np.isnan(fw[0, 4:]).all() and np.isnan(bw[0, :3]).all()
    assert stats["mfma"] == 4 * (625 * 4 + 697 * 2 + 2 * 6)


def test_a_cell_with_a_planned_squaring_between_marked_cells(program):
    _, prog, _ = program
    N, KC, N_T = 64, 1, 3
    H0, Sn, dts, H0f, Sf = scaled_inputs(N, KC, N_T, seed=23, rho=0.97 * THETA_Q)
    dts[1] *= 1.9 / radius(H0, Sn, dts, 0, 1)          # spectral radius 1.9: exponentiated as A / 2 and squared once
    splan = np.array([Q, 1, Q], np.int32)
    rng = np.random.default_rng(8)
    psi0 = rng.normal(size=(KC, N)) + 1j * rng.normal(size=(KC, N))
    U, verdict, stats, fw, bw, prog_ = run_kernel(prog, H0f, Sf, dts, KC, N_T, 1, fuse=3, psi0=psi0, chiT=psi0, want_state=True,
                                                  splan=splan)
    assert list(verdict) == [-1, 0, -1] and list(prog_[0]) == [3]
    x = psi0[0]
    for n in range(N_T):
        ref = scipy.linalg.expm(-1j * dts[n] * (H0[0] + Sn[n]))
        assert np.abs(U[n] - ref).max() < (8e-15 if n == 1 else 2e-15), n
        x = ref @ x
        assert np.abs(fw[0, n + 1] - x).max() < 2e-14 * np.abs(x).max()
    assert stats["mfma"] == 4 * (625 * 2 + 697 + 192 + 2 * 3)


@pytest.mark.parametrize("word,name", [(0, "T16_C16"), (gen_t16q.Q_BIT, "T16Q_C16"), (gen_t16.CERT_BIT, "T16_C16"),
                                       (gen_t16q.Q_BIT | gen_t16.CERT_BIT, "T16Q_C16")])
def test_c16_is_selected_by_the_plan_word_of_the_current_cell(word, name):
    """the two sets' c16 differ by one unit in the last place (1 - 1.1e-16 against 1), which no comparison of results can see: the
    instructions the generator emits for the selection, executed alone with the plan word in s_scur, must leave the bits of the
    right constant in the scalar pair the fourth product adds to the diagonal"""
    import struct
    g = gen_t16q.GenQ()
    k16 = gcn.S(58, 2)
    g.p.salu("s_mov_b32", g.s_scur, word)
    g.load_c16(k16)
    g.p.s_endpgm()
    mem = gcn.GlobalMem()
    a_k, _ = mem.add("kernarg", np.zeros(8, np.uint8))
    e = gcn.Emu(g.p, mem, a_k, nwaves=1, lds_bytes=1024)
    e.run()
    got = struct.unpack("<d", struct.pack("<II", int(e.waves[0].s[58]), int(e.waves[0].s[59])))[0]
    c, cq = gen_t16.t16_coeffs()["C16"], gen_t16q.t16q_coeffs()["C16"]
    assert c != cq
    assert got == (cq if name == "T16Q_C16" else c)
