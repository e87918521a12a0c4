"""The inputs of the table of tests/test_gpu_open_batch.py, checked on the matrix-form reference alone (no GPU): every pulse set
of every case has O(1) signals, so the floor of tol_G never engages, and any two sets of a case differ by far more than the
comparison tolerance in G and in tau -- a kernel that hands set p the pulses, f or storage of set q cannot pass the table.

The references are computed once per case and shared with the GPU tests (``references_of``); nobody modifies them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_reference as orf  # noqa: E402
import test_gpu_open_reference as tgr  # noqa: E402
from open_helpers import TOL_TAU, tol_G  # noqa: E402

P = 4


def pulse_sets(pr):
    """X = [x, 0.5 x, x reversed, 1.3 x] of a case's own pulse vector x.  (-0.8 x is the target's own pulse in several cases:
    the gradient vanishes there.)"""
    x = np.asarray(pr["pulsevals"], dtype=float)
    return np.ascontiguousarray(np.stack([x, 0.5 * x, x[::-1], 1.3 * x]))


_CACHE = {}


def references_of(name):
    """(problem, X [P, L*N_T], [reference of set p]) of a case of test_gpu_open_reference.TABLE"""
    if name not in _CACHE:
        pr, parts = tgr.reference_of(name)
        X = pulse_sets(pr)
        wants = [orf.from_parts(parts, pr, pr["functional"])]
        wants += [orf.evaluate(pr, X[p], functional=pr["functional"]) for p in range(1, P)]
        _CACHE[name] = (pr, X, wants)
    return _CACHE[name]


def many_sets_case():
    """(problem, X [40, L*N_T], reference of set 0, of set 39): d = 5, K = 3, L = 3 -- 360 backward workgroups in one launch"""
    if "many" not in _CACHE:
        from grape_jl_amd import synth
        import open_helpers as oh
        pr = synth.make_open_problem(5, 3, 3, 3, 2, seed=5303)
        pr["functional"], pr["weights"] = 0, np.array([0.5, 1.0, 1.5])
        oh.order_one_states(pr, 5303)
        X = np.ascontiguousarray(np.linspace(0.3, 1.5, 40)[:, None] * pr["pulsevals"][None, :])
        _CACHE["many"] = (pr, X, orf.evaluate(pr, X[0], functional=0), orf.evaluate(pr, X[39], functional=0))
    return _CACHE["many"]


def test_the_ends_of_the_many_sets_case_have_order_one_signals():
    pr, X, want0, want39 = many_sets_case()
    for w in (want0, want39):
        assert np.abs(w["tau"]).min() >= 0.1 and np.abs(w["G"]).max() >= 1e-3
    assert np.abs(want0["G"] - want39["G"]).max() > 100 * tol_G(want0["G"])
    assert np.abs(want0["tau"] - want39["tau"]).max() > 100 * TOL_TAU


@pytest.mark.parametrize("name", tgr.TABLE)
def test_every_set_has_order_one_signals_and_the_sets_differ(name):
    pr, X, wants = references_of(name)
    assert X.shape == (P, pr["pulsevals"].size) and np.array_equal(X[0], pr["pulsevals"])
    tau_min = [float(np.abs(w["tau"]).min()) for w in wants]
    g_max = [float(np.abs(w["G"]).max()) for w in wants]
    print(name, dict(tau_min=tau_min, G_max=g_max))
    assert min(tau_min) >= 0.1
    assert min(g_max) >= 1e-3
    for p in range(P):
        for q in range(p):
            dG = float(np.abs(wants[p]["G"] - wants[q]["G"]).max())
            dtau = float(np.abs(wants[p]["tau"] - wants[q]["tau"]).max())
            assert dG > 100 * max(tol_G(wants[p]["G"]), tol_G(wants[q]["G"])), (p, q, dG)
            assert dtau > 100 * TOL_TAU, (p, q, dtau)
