"""The coefficient set T16Q_* of grape_t18_coeffs.h (second product a Hermitian square: c2 = 0) against the tool that derives
it (tools/t16_coeffs.py, mode q), in 80-digit arithmetic: the header holds a solution of the tool's system to the last printed
digit, its x^15 coefficient vanishes identically, its error on the segment is the 2.19e-16 the header states, and the
rounding figure that selected the branch holds in double precision."""
import os
import re
import sys

import numpy as np
from mpmath import mp, mpf, besselj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import t16_coeffs as T  # noqa: E402

TXT = open(os.path.join(ROOT, "grape.jl_amd", "csrc", "grape_t18_coeffs.h")).read()


def header():
    """(c1..c16, theta) at the tool's 80 digits (other test modules work at other precisions: mp.dps is global)"""
    mp.dps = 80
    c = [mpf(re.search(r"#define\s+T16Q_C%d\s+(-?[\d.eE+-]+)" % i, TXT).group(1)) for i in range(1, 17)]
    return c, mpf(re.search(r"#define\s+T16Q_THETA\s+([\d.]+)", TXT).group(1))


def test_header_set_solves_the_system_of_the_tool():
    C, THETA = header()
    assert THETA == mpf("1.11") and C[1] == 0
    u0 = [C[i] for i in T.QIDX]
    u, err = T.solve_q(T.q_target(THETA), u0)
    assert err < mpf(10) ** -70
    # (20 significant digits printed: half a unit of the last one, relative to each coefficient)
    assert all(abs(a - b) <= abs(b) * mpf(10) ** -19 / 2 for a, b in zip(u, u0))
    p = T.t16_poly(T.q_full(u))
    assert p[15] == 0 and abs(p[16] - u[0] ** 4) < mpf(10) ** -70


def test_error_on_the_segment():
    C, THETA = header()
    err = T.seg_error(C, THETA, n=401)
    assert err < mpf("2.2e-16") and err > 2 * besselj(15, THETA) * mpf("0.99")     # the missing T15 term, nothing else of weight
    assert 2 * besselj(15, THETA) < mpf("2.2e-16")


def test_rounding_in_double_at_the_edge_of_the_segment():
    """max element error against the 80-bit reference, N = 64, rho = 1.11, three matrices: 2.0e-16 measured when the branch was
    selected (the branches the tool rejects: 1.8e-15)"""
    C, THETA = header()
    (e, n2), = T.q_rounding([[float(x) for x in C]], THETA)
    assert e < 3e-16 and n2 < 5e-16, (e, n2)
