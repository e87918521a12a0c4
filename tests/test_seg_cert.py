"""The three-moment certificate of the degree-15 derivative series (t16_seg_certified, grape_kernels.hip.h), restated in
numpy as the device evaluates it (tests/seg_cert_reference.py), against the eigenvalues: it never certifies a spectrum whose
radius exceeds the segment -- random and adversarial spectra -- its tables reproduce the moments, and it certifies every
cell of a problem shaped like the benchmark's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from grape_jl_amd import synth  # noqa: E402
import seg_cert_reference as sc  # noqa: E402

TH = sc.THETA15


def test_the_segment_is_the_one_the_header_names():
    assert (sc.DEG15, TH) == (15, 1.11)
    assert [d for d, _ in sc.header_sets()] == sorted(d for d, _ in sc.header_sets())   # (tables are indexed by M - ECON_MINDEG)


def test_random_hermitian_matrices_are_never_certified_beyond_the_segment():
    rng = np.random.default_rng(5)
    seen = {True: 0, False: 0}
    for i, f in enumerate(np.linspace(0.9, 1.2, 601)):
        X = rng.normal(size=(64, 64)) + 1j * rng.normal(size=(64, 64))
        lam = np.linalg.eigvalsh((X + X.conj().T) / 2)
        lam *= f * TH / np.abs(lam).max()
        rho = np.abs(lam).max()
        ok = sc.certified_spectrum(lam)
        assert not (ok and rho > TH), (f, rho)
        seen[ok] += 1
    # (not vacuous: on a semicircle the bound is some 6 % above the radius, so the lowest tenth of the scan is certified)
    assert seen[True] > 50 and seen[False] > 300


def adversarial(N=64):
    """unit-radius spectra that press on each inequality"""
    out = {}
    bulk = np.linspace(-0.35, 0.35, N)
    for mult in (1, 2, 8):
        lam = bulk.copy()
        lam[:mult] = [(-1.0) ** j for j in range(mult)]
        out[f"top eigenvalue x{mult} over a flat bulk"] = lam
    out["flat"] = np.linspace(-1.0, 1.0, N)
    r1 = np.zeros(N)
    r1[0] = -1.0
    out["rank one"] = r1
    out["all equal in modulus"] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    out["N = 49 padded"] = np.concatenate([np.linspace(-1.0, 0.8, 49), np.zeros(N - 49)])
    out["two levels"] = np.concatenate([np.full(N // 2, 1.0), np.full(N - N // 2, 0.97)])
    out["bulk just below the top"] = np.concatenate([[1.0], np.full(N - 1, 0.999)])
    return out


@pytest.mark.parametrize("name", list(adversarial()))
def test_adversarial_spectra_are_never_certified_beyond_the_segment(name):
    lam0 = adversarial()[name]
    certified_below = False
    for f in np.concatenate([np.linspace(0.5, 0.99, 50), np.linspace(0.99, 1.01, 2001), np.linspace(1.01, 1.6, 60)]):
        lam = lam0 * (f * TH)
        ok = sc.certified_spectrum(lam)
        assert not (ok and np.abs(lam).max() > TH), (name, f)
        certified_below = certified_below or ok
    assert certified_below                                   # (every one of them passes once it is small enough: m4 <= theta^4)


def test_nan_and_empty_moments():
    nan = float("nan")
    assert not sc.seg_certified(nan, 1.0, 1.0, 1.0, 1.0, 1.0)
    assert not sc.seg_certified(2.0, 2.0, nan, 1.0, 1.0, 1.0)
    assert not sc.seg_certified(2.0, 2.0, 1.0, 1.0, nan, 1.0)
    assert not sc.seg_certified(2.0, 2.0, 1.0, 1.0, 1.0, 1.0, dt=nan)
    assert sc.seg_certified(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_the_bound_is_never_below_the_spectral_radius_and_tighter_than_single_moments():
    pr = synth.make_problem(64, 2, 40, 2, seed=7)
    for k in range(2):
        for n in range(0, 40, 3):
            lam = sc.cell_spectrum(pr, k, n)
            m4, m8, m12 = sc.moments(lam)
            b = sc.three_moment_bound(lam)
            assert np.abs(lam).max() <= b <= m12 ** (1 / 12) + 1e-3 < m8 ** (1 / 8)


@pytest.mark.parametrize("N,L", [(64, 2), (49, 2), (64, 1)])
def test_tables_against_the_moments_of_the_eigenvalues(N, L):
    pr = synth.make_problem(N, L, 12, 2, seed=N + L)
    for k in range(2):
        t4, t8, t12, e4, e8, e12 = sc.seg_tables([pr["H0"][k]] + list(pr["Hc"]))
        assert (len(t4), len(t8), len(t12)) == ((15, 45, 91) if L == 2 else (5, 9, 13))
        for n in range(12):
            H, dt, e = sc.cell_generator(pr, k, n)
            m4, m8, m12 = sc.moments(np.linalg.eigvalsh(H))
            for t, ex, m in ((t4, e4, m4), (t8, e8, m8), (t12, e12, m12)):
                p, S = sc.poly(t, ex, e)
                assert abs(p - m) <= 1e-12 * m
                assert abs(p - m) <= 1e-3 * sc.G * S              # (what the guard of the device's test rests on)


def test_every_cell_of_a_benchmark_like_problem_is_certified():
    """synth.make_problem(64, 2, ...): drift members, controls and pulse distribution of C3.  On C3 itself (16 trajectories,
    all 1000 steps) the bound is at most 1.11 on 99.8 % of the cells and at most 1.12 on all of them; the seed below is one
    whose 240 cells all lie below 1.11 (worst bound 1.097, checked here from the eigenvalues), and the device's test, from
    the tables, must then certify every one"""
    seed = 2
    K, N_T = 4, 60
    pr = synth.make_problem(64, 2, N_T, K, seed=seed)
    worst = 0.0
    for k in range(K):
        t4, t8, t12, e4, e8, e12 = sc.seg_tables([pr["H0"][k]] + list(pr["Hc"]))
        for n in range(N_T):
            H, dt, e = sc.cell_generator(pr, k, n)
            (p4, S4), (p8, S8), (p12, S12) = sc.poly(t4, e4, e), sc.poly(t8, e8, e), sc.poly(t12, e12, e)
            lam = np.linalg.eigvalsh(H) * dt
            assert np.abs(lam).max() < TH
            assert sc.seg_certified(p4, S4, p8, S8, p12, S12, dt), (k, n)
            worst = max(worst, sc.three_moment_bound(lam))
    assert worst <= TH, worst
