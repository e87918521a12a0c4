"""The trace tables behind the pre-launch certificate of the four-product cell (grape.jl_amd/csrc/grape_cert.hip.h,
t16_plan_kernel): tr H^8 and tr H^6 of H = H0 + sum_l e_l C_l as polynomials in e, restated in numpy the way the
library builds them -- coefficient matrices of H^2, H^3 = H^2 H, H^4 = H^2 H^2, pairwise traces -- and checked against the
moments of the eigenvalues.  What the rigorous margin of the certificate rests on: |p8 - m8| <= 2^-30 S8 with
S8 = sum |t8[al]| |e^al| on every sample, far below the 1e-6 the test leaves."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from grape_jl_amd import synth  # noqa: E402


def monomials(M, d):
    """exponent tuples of degree d in M variables, lexicographic with the larger exponent of the earlier variable first
    (CertMonomials)"""
    out = []

    def gen(a, left, cur):
        if a == M - 1:
            out.append(tuple(cur + [left]))
            return
        for e in range(left, -1, -1):
            gen(a + 1, left - e, cur + [e])
    gen(0, d, [])
    return out


def trace_tables(ops):
    """ops [M][N][N] = (H0, C_1 .. C_L) -> (t8, t6, exponents of e_1 .. e_L for t8 | t6)"""
    M = len(ops)
    add = lambda x, y: tuple(a + b for a, b in zip(x, y))  # noqa: E731
    unit = lambda a: tuple(1 if i == a else 0 for i in range(M))  # noqa: E731
    m2, m3, m4, m6, m8 = (monomials(M, d) for d in (2, 3, 4, 6, 8))
    Z = lambda: np.zeros_like(ops[0])  # noqa: E731
    M2 = {k: Z() for k in m2}
    for a in range(M):
        for b in range(M):
            M2[add(unit(a), unit(b))] += ops[a] @ ops[b]
    M3 = {k: Z() for k in m3}
    for k2 in m2:
        for c in range(M):
            M3[add(k2, unit(c))] += M2[k2] @ ops[c]
    M4 = {k: Z() for k in m4}
    for ka in m2:
        for kb in m2:
            M4[add(ka, kb)] += M2[ka] @ M2[kb]
    t8 = {k: 0.0 for k in m8}
    for ka in m4:
        for kb in m4:
            t8[add(ka, kb)] += np.sum(M4[ka] * M4[kb].T).real
    t6 = {k: 0.0 for k in m6}
    for ka in m3:
        for kb in m3:
            t6[add(ka, kb)] += np.sum(M3[ka] * M3[kb].T).real
    return (np.array([t8[k] for k in m8]), np.array([t6[k] for k in m6]),
            np.array([k[1:] for k in m8], int).reshape(len(m8), M - 1), np.array([k[1:] for k in m6], int).reshape(len(m6), M - 1))


def evaluate(t, ex, e):
    """(p, S) = (sum t[al] e^al, sum |t[al]| |e^al|)"""
    mono = np.prod(np.asarray(e)[None, :] ** ex, axis=1)
    return float(np.sum(t * mono)), float(np.sum(np.abs(t) * np.abs(mono)))


def test_monomial_counts():
    # L = 2: 6 + 10 + 15 coefficient matrices, 45 + 28 coefficients
    assert [len(monomials(3, d)) for d in (2, 3, 4, 6, 8)] == [6, 10, 15, 28, 45]
    assert [len(monomials(5, d)) for d in (2, 3, 4, 6, 8)] == [15, 35, 70, 210, 495]


@pytest.mark.parametrize("N,L", list(itertools.product((8, 64), (1, 2, 3))) + [(8, 4)])   # L = 4: GRAPE_CERT_LMAX, 495 + 210 coefficients
def test_tables_against_the_moments_of_the_eigenvalues(N, L):
    pr = synth.make_problem(N, L, 4, 2, seed=900 + N + L)
    rng = np.random.default_rng(N + L)
    worst = 0.0
    for k in range(2):
        ops = [pr["H0"][k]] + [pr["Hc"][l] for l in range(L)]
        t8, t6, ex8, ex6 = trace_tables(ops)
        # pulse values of the benchmarks are 0.1 +- 0.2: samples up to ten times that range, either sign, and the corners
        samples = [3.0 * (2.0 * rng.random(L) - 1.0) for _ in range(12)] + [0.3 * (2.0 * rng.random(L) - 1.0) for _ in range(6)]
        samples += [np.zeros(L), np.full(L, 3.0), np.full(L, -3.0)]
        for e in samples:
            lam = np.linalg.eigvalsh(ops[0] + sum(e[l] * ops[1 + l] for l in range(L)))
            m8, m6 = np.sum(lam ** 8), np.sum(lam ** 6)
            p8, S8 = evaluate(t8, ex8, e)
            p6, _ = evaluate(t6, ex6, e)
            assert abs(p8 - m8) <= 1e-12 * m8 and abs(p6 - m6) <= 1e-12 * m6, (e, p8 / m8 - 1, p6 / m6 - 1)
            assert abs(p8 - m8) <= 2.0 ** -30 * S8
            worst = max(worst, abs(p8 - m8) / m8, abs(p6 - m6) / m6)
    print("worst relative error of p8, p6: %.2e" % worst)
