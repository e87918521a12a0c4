"""The segment certificate of the economized derivative series restated in numpy (t16_seg_certified and the tables of
grape_cert.hip.h): three even moments m4, m8, m12 of the eigenvalues of H dt place the spectral radius below theta when

    m4 <= theta^4     or     m8 < theta^4 m4   and   (m12 - theta^12)(m4 - theta^4) < (m8 - theta^8)^2,

every moment taken at the unfavourable end of p dt^k -+ 2^-30 S dt^k and a relative 1e-6 on each inequality.  Shared by
the CPU tests of the inequality and the GPU tests of the route."""
import os
import re

import numpy as np

from test_cert_table import monomials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_sets():
    """[(degree, theta)] of grape_econ_coeffs.h"""
    text = open(os.path.join(ROOT, "grape.jl_amd", "csrc", "grape_econ_coeffs.h")).read()
    degs = [int(x) for x in re.search(r"ECON_DEG\[\d+\] = \{([^}]*)\}", text).group(1).split(",")]
    thetas = [float(x) for x in re.search(r"ECON_THETAS\[\d+\] = \{([^}]*)\}", text).group(1).split(",")]
    assert float(re.search(r"#define ECON_SEG_THETA ([0-9.]+)", text).group(1)) == thetas[0]
    return list(zip(degs, thetas))


DEG15, THETA15 = header_sets()[0]
G = 2.0 ** -30


def seg_certified(p4, S4, p8, S8, p12, S12, dt=1.0, theta=THETA15):
    """the device's test, operation by operation (NaN fails)"""
    th2 = theta * theta
    th4 = th2 * th2
    th8 = th4 * th4
    th12 = th8 * th4
    dt2 = dt * dt
    dt4 = dt2 * dt2
    dt8 = dt4 * dt4
    dt12 = dt8 * dt4
    m4lo, m4hi = (p4 - G * S4) * dt4, (p4 + G * S4) * dt4
    m8lo, m8hi = (p8 - G * S8) * dt8, (p8 + G * S8) * dt8
    m12hi = (p12 + G * S12) * dt12
    if m4hi * (1.0 + 1e-6) <= th4:
        return True
    if not (m8hi * (1.0 + 1e-6) < th4 * m4lo):
        return False
    lo, hi = m8lo - th8, m8hi - th8
    gap = lo if lo > 0.0 else -hi if hi < 0.0 else 0.0
    lhs = (m12hi - th12) * (m4hi - th4)
    return bool((lhs * (1.0 + 1e-6) if lhs > 0.0 else lhs) < gap * gap)


def moments(lam):
    lam = np.asarray(lam, dtype=np.float64)
    return tuple(float(np.sum(lam ** p)) for p in (4, 8, 12))


def certified_spectrum(lam, theta=THETA15):
    """the test on the exact moments of a spectrum (guards on the moments themselves: every term is >= 0)"""
    m4, m8, m12 = moments(lam)
    return seg_certified(m4, m4, m8, m8, m12, m12, 1.0, theta)


def three_moment_bound(lam, step=1e-3):
    """the smallest theta on a grid of `step` above rho from which the test certifies the spectrum"""
    rho = float(np.abs(lam).max())
    th = rho
    while not certified_spectrum(lam, th):
        th += step
        assert th < 2.0 * rho + 1.0
    return th


def seg_tables(ops):
    """ops [M][N][N] = (H0, C_1 .. C_L) -> (t4, t8, t12, exponents of e_1 .. e_L of t4, t8, t12): coefficient matrices of
    H^2, H^3 = H^2 H, H^4 = H^2 H^2, H^6 = H^3 H^3 and pairwise traces, in the library's order"""
    M = len(ops)
    add = lambda x, y: tuple(a + b for a, b in zip(x, y))  # noqa: E731
    unit = lambda a: tuple(1 if i == a else 0 for i in range(M))  # noqa: E731
    mons = {d: monomials(M, d) for d in (2, 3, 4, 6, 8, 12)}
    Z = lambda: np.zeros_like(ops[0])  # noqa: E731
    M2 = {k: Z() for k in mons[2]}
    for a in range(M):
        for b in range(M):
            M2[add(unit(a), unit(b))] += ops[a] @ ops[b]
    M3 = {k: Z() for k in mons[3]}
    for k2 in mons[2]:
        for c in range(M):
            M3[add(k2, unit(c))] += M2[k2] @ ops[c]
    M4 = {k: Z() for k in mons[4]}
    for ka in mons[2]:
        for kb in mons[2]:
            M4[add(ka, kb)] += M2[ka] @ M2[kb]
    M6 = {k: Z() for k in mons[6]}
    for ka in mons[3]:
        for kb in mons[3]:
            M6[add(ka, kb)] += M3[ka] @ M3[kb]

    def traces(mats, deg):
        t = {k: 0.0 for k in mons[deg]}
        for ka, A in mats.items():
            for kb, B in mats.items():
                t[add(ka, kb)] += np.sum(A * B.T).real
        return np.array([t[k] for k in mons[deg]])
    ex = {d: np.array([k[1:] for k in mons[d]], dtype=np.int64).reshape(len(mons[d]), M - 1) for d in (4, 8, 12)}
    return traces(M2, 4), traces(M4, 8), traces(M6, 12), ex[4], ex[8], ex[12]


def poly(t, ex, e):
    """(p, S) = (sum t e^ex, sum |t| |e^ex|), summed in table order"""
    p = S = 0.0
    for c, x in zip(t, ex):
        mono = 1.0
        for el, q in zip(e, x):
            mono *= float(el) ** int(q)
        p += c * mono
        S += abs(c) * abs(mono)
    return p, S


def cell_generator(pr, k, n):
    """H of cell (k, n) and its step"""
    L, N_T = pr["L"], pr["N_T"]
    Hc = pr["Hc"][k] if pr["Hc"].ndim == 4 else pr["Hc"]
    e = [pr["pulsevals"][l * N_T + n] for l in range(L)]
    H = pr["H0"][k] + sum(e[l] * Hc[l] for l in range(L))
    return H, float(pr["tlist"][n + 1] - pr["tlist"][n]), e


def cell_spectrum(pr, k, n):
    H, dt, _ = cell_generator(pr, k, n)
    return np.linalg.eigvalsh(H) * dt
