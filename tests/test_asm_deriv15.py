"""The degree-15 polynomial of the economized derivative series (grape_econ_coeffs.h: spectral radius <= 1.11) in the
emulated derivative kernels deriv3_asm and deriv3s_asm (tests/test_asm_deriv3.py has the harness): a batch -- for the
streamed kernel, the four batches a workgroup walks together -- whose cells are all certified for the short segment stops
pass 1 after 14 orders and runs 15 in pass 2; a single cell of the next segment makes its batch run degree 16; a batch
whose Taylor terms fall below the tolerance before 14 orders keeps the Taylor scalars bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_asm_deriv3 as t3  # noqa: E402
from test_asm_deriv3 import gen_d3, gen_d3s  # noqa: E402


def inputs(N, L, groups, seed):
    """cells per group: the first all inside 1.11, the second with one cell at 1.25, the third with steps so short that the
    Taylor sum converges before 14 orders; returns the inputs and the degree every cell is certified for"""
    N_T = sum(groups)
    d = t3.make_inputs(N, 1, L, N_T, seed=seed)
    rng = np.random.default_rng(seed + 1)
    etabs = t3.econ_tables()
    th15, th16 = etabs[15][0], etabs[16][0]
    assert (th15, th16) == (1.11, 1.36)
    target = 0.95 + 0.15 * rng.random(N_T)
    odd = groups[0] + groups[1] // 3
    target[odd] = 1.25
    target[groups[0] + groups[1]:] = 0.15
    deg = np.zeros(N_T, int)
    for n in range(N_T):
        H = d["H0"][0] + sum(d["eps"][l, n] * d["Hc"][0, l] for l in range(L))
        d["dts"][n] = target[n] / np.abs(np.linalg.eigvalsh(H)).max()
        deg[n] = 15 if target[n] <= th15 else 16
    assert (deg == 16).sum() == 1
    return d, deg, odd


def batch_degrees(deg, N_T):
    """deriv_econ_kernel's rule: a batch takes the largest degree of its cells"""
    return np.array([[deg[16 * b:16 * b + 16].max() for b in range((N_T + 15) // 16)]], np.int32)


@pytest.fixture(scope="module")
def program():
    return gen_d3.generate()


@pytest.fixture(scope="module")
def program_s():
    return gen_d3s.generate()


def check(tg, flags, stats, d, econ, orders, want, group_wpt=None):
    ref, orders_r = t3.series_reference(d, group_wpt=group_wpt, econ=econ)
    assert (orders_r == orders).all() and (orders[want > 0] == want[want > 0]).all() and (orders[want < 0] < 14).all(), (orders, want)
    assert np.abs(tg - ref).max() < 2e-15 * max(1.0, np.abs(ref).max()) * 8, np.abs(tg - ref).max()
    fre = t3.frechet_reference(d)
    assert np.abs(tg - fre).max() < 1e-13, np.abs(tg - fre).max()
    assert flags[0] == 0 and flags[7] == 0
    N_T = d["N_T"]
    cells = np.array([[min(16, N_T - 16 * b) for b in range((N_T + 15) // 16)]])
    assert int(stats[:, 8].sum()) == int((orders * cells).sum())


def test_one_wave_kernel_degree_15_mixed_and_converged_batches(program):
    _, prog, _ = program
    d, deg, odd = inputs(64, 2, (16, 16, 9), seed=21)
    econ = batch_degrees(deg, d["N_T"])
    assert econ.tolist() == [[15, 16, 15]] and (econ == t3.certified_batches(d, (15, 16))).all()
    tg, flags, stats, _ = t3.run_kernel(prog, d, 1, 1, econ=econ)
    _, orders = t3.series_reference(d, econ=econ)
    check(tg, flags, stats, d, econ, orders, np.array([[15, 16, -1]]))
    # the converged batch: the Taylor sum's bits, whatever it is certified for
    tg_t, _, _, _ = t3.run_kernel(prog, d, 1, 1)
    assert np.array_equal(tg[:, :, 32:].view(np.float64), tg_t[:, :, 32:].view(np.float64))
    assert not np.array_equal(tg[:, :, :32].view(np.float64), tg_t[:, :, :32].view(np.float64))


def test_streamed_kernel_degree_15_mixed_and_converged_groups(program_s):
    _, prog, _ = program_s
    d, deg, odd = inputs(50, 1, (64, 64, 9), seed=22)
    econ = batch_degrees(deg, d["N_T"])
    assert econ.tolist() == [[15] * 4 + [15, 16, 15, 15] + [15]]
    tg, flags, stats, _ = t3.run_kernel(prog, d, 1, 1, lds_bytes=gen_d3s.LDS_BYTES, econ=econ)
    _, orders = t3.series_reference(d, group_wpt=1, econ=econ)
    check(tg, flags, stats, d, econ, orders, np.array([[15] * 4 + [16] * 4 + [-1]]), group_wpt=1)
    tg_t, _, _, _ = t3.run_kernel(prog, d, 1, 1, lds_bytes=gen_d3s.LDS_BYTES)
    assert np.array_equal(tg[:, :, 128:].view(np.float64), tg_t[:, :, 128:].view(np.float64))
