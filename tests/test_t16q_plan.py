"""Which cells the plan marks for the Hermitian-square path of expm_t16q_asm (bit 9 of the plan word), on the CPU: the
restatement of t16_plan_kernel's arithmetic (tests/t16q_reference.py) against the moments of the eigenvalues on cells 1 %
inside and outside each of the two edges that decide -- the three-moment bound at 1.11 and the certificate's inequality at
1.36 -- and, in that restatement, the independence of the route's bit from the switches of the two other users of the trace
tables (and of their outputs from the route's switch).  This file checks the ARITHMETIC and the intended control flow as
restated in Python; it never runs t16_plan_kernel and cannot see a coupling inside it -- that is what
tests/test_gpu_t16q.py::test_the_route_does_not_depend_on_the_other_switches is for."""
import itertools

import numpy as np
import pytest

import seg_cert_reference as sc
import t16_route_reference as R
import t16q_reference as Q
from grape_jl_amd import synth


def one_cell(H, dt, C=None):
    """a problem of one trajectory and one time step with generator H (+ 0 * C)"""
    N = H.shape[0]
    C = np.zeros_like(H) if C is None else C
    return dict(N=N, L=1, N_T=1, K=1, H0=H[None], Hc=C[None], psi0=synth.unit_vectors(1, 1, N), target=synth.unit_vectors(2, 1, N),
                pulsevals=np.zeros(1), weights=np.ones(1), tlist=np.array([0.0, dt]))


def marked(pr, **kw):
    return bool(Q.plan_words(pr, **kw)[0][0, 0] & Q.Q_BIT)


@pytest.mark.parametrize("N", [64, 49])
@pytest.mark.parametrize("f,want", [(0.99, True), (1.01, False)])
def test_cells_at_the_edge_of_the_segment(N, f, want):
    """a semicircle-like spectrum scaled so that the three-moment bound is f * 1.11: inside the range of the four products
    either way (m8^(1/8) <= 1.25 rho there), so condition (c) alone decides"""
    H = synth.gue(40 + N, N)
    lam = np.linalg.eigvalsh(H)
    dt = f * Q.THETA_Q / sc.three_moment_bound(lam, step=1e-4)
    assert np.sum((lam * dt) ** 8) ** 0.125 < 0.97 * R.THETA
    pr = one_cell(H, dt)
    assert R.plan_squarings(R.plan_estimate(R.operators(pr, 0), R.amplitudes(pr, 0), dt))[0] == 0
    assert sc.certified_spectrum(lam * dt) == want
    assert marked(pr) == want


@pytest.mark.parametrize("f,want", [(0.99, True), (1.01, False)])
def test_cells_at_the_edge_of_the_four_products(f, want):
    """a two-point spectrum +-rho: m8^(1/8) = N^(1/8) rho = 1.68 rho at N = 64, so at m8^(1/8) = f * 1.36 the radius is 0.8,
    far inside the segment -- condition (b) alone decides, and a marked cell is one the cell's own bound would have passed"""
    N = 64
    V = np.linalg.qr(synth.gue(5, N))[0]
    H = (V * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)) @ V.conj().T
    H = 0.5 * (H + H.conj().T)
    dt = f * R.THETA / N ** 0.125
    lam = np.linalg.eigvalsh(H) * dt
    assert sc.certified_spectrum(lam)                          # (c) holds on both sides
    assert abs(np.sum(lam ** 8) ** 0.125 / R.THETA - f) < 1e-9
    pr = one_cell(H, dt)
    # (the plan's estimate is m8^(1/8) / 1.17 for a single operator: it plans a squaring from m8^(1/8) = 1.345 on, so this edge
    # is met at s = 0 only where the estimate is off, as in the inputs of t16_route_reference.py, or without planned squarings,
    # GRAPE_EXPM_SQ=0 -- taken here)
    assert marked(pr, sq_on=False) == want
    # a marked cell is one the certificate passes (beyond the edge this spectrum is still passed by the cell's 1-norm test,
    # A^2 = -rho^2: not what the plan can know from the traces)
    assert R.decide(pr, sq_on=False)["kind"][0][0] == (R.CERTIFIED if want else R.PASSED)


def test_a_cell_with_planned_squarings_is_never_marked():
    H = synth.gue(3, 64)
    pr = one_cell(H, 1.9 / np.abs(np.linalg.eigvalsh(H)).max())
    splan = Q.plan_words(pr)[0]
    assert splan[0, 0] & 0xFF == 1 and not splan[0, 0] & Q.Q_BIT


def test_the_three_users_of_the_tables_do_not_see_each_other():
    """cells on both sides of both edges and one with a planned squaring, all eight settings of the three switches: the route's
    bits depend on its own switch only, the certified bits, the segment plan and the verdicts the certificate writes likewise"""
    pr = synth.make_problem(64, 2, 8, 2, seed=2)
    d = np.diff(pr["tlist"])
    b = [sc.three_moment_bound(sc.cell_spectrum(pr, 0, n)) for n in range(8)]
    d[1] = 1.02 * Q.THETA_Q / b[1]
    d[3] = 1.30 / b[3]
    d[5] = 1.9 / b[5]
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(d)])
    res = {sw: Q.plan_words(pr, *sw) for sw in itertools.product((False, True), repeat=3)}
    ref = res[(True, True, True)]
    qbits = ref[0] & Q.Q_BIT
    assert qbits[:, [0, 2, 4, 6, 7]].all() and not qbits[:, [1, 3, 5]].any()
    assert (ref[0][:, 5] & 0xFF == 1).all()
    for (cert, seg, q), (splan, segplan, verdict) in res.items():
        assert np.array_equal(splan & 0xFF, ref[0] & 0xFF)
        assert np.array_equal(splan & Q.Q_BIT, qbits if q else 0 * qbits)
        assert np.array_equal(splan & Q.CERT_BIT, ref[0] & Q.CERT_BIT if cert else 0 * qbits)
        assert (segplan is None) == (not seg) and (not seg or np.array_equal(segplan, ref[1]))
        # the verdict word: 0 from the certificate or from this route; a marked cell is one the certificate passes at s = 0
        want = np.where(((splan & Q.CERT_BIT) != 0) | ((splan & Q.Q_BIT) != 0), 0, -1)
        assert np.array_equal(verdict, want)
    # condition (b): every marked cell is certified by the certificate too -- the hand-over list cannot change
    assert ((ref[0] & Q.CERT_BIT) != 0)[qbits != 0].all()
