"""Which cells take the Hermitian-square path of expm_t16q_asm, restated in numpy from t16_plan_kernel
(grape.jl_amd/csrc/grape_kernels.hip.h): a cell is marked (bit 9 of its plan word, verdict 0 written by the plan) iff

  (a) the plan gave it no squarings,
  (b) it passes the certificate's inequality for 1.36 at s = 0:  (p8 + 2^-30 S8) dt^8 (1 + 1e-6) <= 1.36^8  and  p6 >= 0,
  (c) the three moments certify its spectral radius for 1.11 (t16_seg_certified),

from the trace tables of its generator class.  The three users of the tables have a switch each (certificate: bit 8 and the
verdict it implies; segment certificate: segplan; this route: bit 9) and nobody's output depends on another's switch --
plan_words() below follows the kernel's control flow switch by switch.  Used by tests/test_t16q_plan.py (CPU) and
tests/test_gpu_t16q.py (GPU)."""
import numpy as np

import seg_cert_reference as sc
import t16_route_reference as R
from test_cert_table import evaluate, trace_tables

THETA_Q = sc.THETA15          # the segment the T16Q_* coefficients were made for is the one the plan certifies
CERT_BIT, Q_BIT = 0x100, 0x200
G = 2.0 ** -30


def cert_inequality(p8, S8, p6, dt, s):
    """t16_certified"""
    return bool((p8 + G * S8) * dt ** 8 * (1.0 + 1e-6) <= (R.THETA * 2.0 ** s) ** 8 and p6 >= 0.0)


def plan_words(pr, cert_use=True, seg_use=True, q_use=True, sq_on=True):
    """(splan [KC][N_T], segplan [KC][N_T] or None, verdict written by the plan [KC][N_T]: 0 or -1 for "left to the cell")"""
    cls, reps = R.classes(pr)
    KC, N_T = len(reps), len(pr["tlist"]) - 1
    dts = np.diff(pr["tlist"])
    L = pr["pulsevals"].size // N_T
    have86 = cert_use or q_use          # what grape_create builds: t8 | t6 for the certificate or this route ...
    have412 = seg_use or q_use          # ... t4 | t12 for the segment certificate or this route
    splan = np.zeros((KC, N_T), int)
    segplan = np.zeros((KC, N_T), int) if seg_use else None
    verdict = np.full((KC, N_T), -1)
    for kc, k in enumerate(reps):
        ops = R.operators(pr, k)
        t8, t6, ex8, ex6 = trace_tables(ops)
        t4, t8s, t12, ex4, ex8s, ex12 = sc.seg_tables(ops)
        for n in range(N_T):
            e, dt = R.amplitudes(pr, n), dts[n]
            s, out, _ = R.plan_squarings(R.plan_estimate(ops, e, dt), sq_on)
            word = s
            p8 = S8 = p6 = None
            if have86 and (cert_use or q_use):
                (p8, S8), (p6, _) = evaluate(t8, ex8, e), evaluate(t6, ex6, e)
                if cert_use and cert_inequality(p8, S8, p6, dt, s):
                    verdict[kc, n] = 0
                    word |= CERT_BIT
            if have412 and (seg_use or q_use):
                seg = False
                if s == 0:
                    if p8 is None:
                        p8, S8 = sc.poly(t8s, ex8s, e)
                    (p4, S4), (p12, S12) = sc.poly(t4, ex4, e), sc.poly(t12, ex12, e)
                    seg = sc.seg_certified(p4, S4, p8, S8, p12, S12, dt)
                if seg_use:
                    segplan[kc, n] = int(seg)
                if q_use and seg and cert_inequality(p8, S8, p6, dt, 0):
                    verdict[kc, n] = 0
                    word |= Q_BIT
            splan[kc, n] = word
    return splan, segplan, verdict


def margins(pr):
    """[KC][N_T] distance of every cell from the two edges that decide bit 9, from the eigenvalues: three-moment bound / 1.11 - 1
    and m8^(1/8) / 1.36 - 1"""
    cls, reps = R.classes(pr)
    N_T = len(pr["tlist"]) - 1
    dts = np.diff(pr["tlist"])
    d11, d136 = np.zeros((len(reps), N_T)), np.zeros((len(reps), N_T))
    for kc, k in enumerate(reps):
        ops = R.operators(pr, k)
        for n in range(N_T):
            e = R.amplitudes(pr, n)
            lam = np.linalg.eigvalsh(ops[0] + sum(e[l] * ops[1 + l] for l in range(len(e)))) * dts[n]
            d11[kc, n] = sc.three_moment_bound(lam) / THETA_Q - 1.0
            d136[kc, n] = np.sum(lam ** 8) ** 0.125 / R.THETA - 1.0
    return d11, d136


def expected_q(pr, margin=0.005):
    """[KC][N_T] bool: the cells the route takes, decided from the eigenvalues; asserts that no cell is within `margin` of an
    edge that decides (a cell beyond 1.11 by the margin is out whatever its distance from 1.36)"""
    d11, d136 = margins(pr)
    splan, _, _ = plan_words(pr)
    sq = splan & 0xFF
    inside11, inside136 = d11 <= -margin, d136 <= -margin
    decided = (sq > 0) | (d11 >= margin) | (inside11 & (inside136 | (d136 >= margin)))
    assert decided.all(), (d11[~decided], d136[~decided])
    q = (sq == 0) & inside11 & inside136
    assert np.array_equal(q, (splan & Q_BIT) != 0)          # the tables say what the eigenvalues say
    return q
