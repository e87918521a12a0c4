"""grape_open_eval_batch (csrc/grape_lindblad_batch.hip.h): pulse sets side by side on an open-system handle --
needs an MI355X.  tests/test_open_batch_reference.py checks the inputs of the table on the reference alone (O(1) signals in
every set, sets that differ by far more than the tolerance).  Tolerances are the project's:
    |dJ| <= 1e-12,  |dtau_k| <= 1e-12,  ||dG||_inf <= 1e-10 ||G||_inf
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
import open_reference as orf  # noqa: E402
import test_gpu_open_reference as tgr  # noqa: E402
import test_open_batch_reference as tbr  # noqa: E402
from open_helpers import TOL_J, TOL_TAU, tol_G  # noqa: E402
from test_gpu_open_reference import build_case  # noqa: E402,F401  (the cases of the table; cached through tgr.reference_of)

pytestmark = pytest.mark.gpu

SM, SS, RE = 0, 1, 2
_open = tgr._open


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


def _bits(a, b):
    """(J, G, tau) triples with the same bits"""
    return all((x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _row(out, p):
    J, G, tau = out
    return J[p], None if G is None else G[p], tau[p]


def _agrees(got, want, label):
    """one set against (J, G, tau) of a reference or of grape_eval: the project's tolerances"""
    return oh.assert_open_agrees(dict(J=got[0], G=got[1], tau=got[2]), dict(J=want[0], G=want[1], tau=want[2]), label)


def _five(pr):
    x = pr["pulsevals"]
    return np.ascontiguousarray(np.stack([x, 0.5 * x, x[::-1], 1.3 * x, 0.7 * x]))


# ---- 1. the table against the matrix-form reference --------------------------------------------------------------------------
@pytest.mark.parametrize("name", tgr.TABLE)
def test_table_against_the_matrix_form_reference(g, name):
    pr, X, wants = tbr.references_of(name)
    for w in wants:
        oh.assert_order_one(w)
    with _open(g, pr) as h:
        out = h.open_eval_batch(X)
        info = h.open_batch_info()
    assert out[0].shape == (4,) and out[1].shape == X.shape and out[2].shape == (4, pr["H0"].shape[0])
    assert info["sets_per_group"] == 4 and info["groups"] == 1 and info["bytes"] > 0
    for p, w in enumerate(wants):
        _agrees(_row(out, p), (w["J"], w["G"], w["tau"]), f"{name} set {p}")
    K, L, N_T = pr["H0"].shape[0], X.shape[1] // 3, 3
    if tgr.CASES[name].get("long_step"):
        assert info["series_steps"] > 4 * (K + K * L) * N_T
    else:
        assert info["series_steps"] >= 4 * (K + K * L) * N_T


# ---- 2. against the handle's own grape_eval ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tgr.TABLE)
def test_table_against_grape_eval_of_the_same_handle(g, name):
    pr, X, _ = tbr.references_of(name)
    with _open(g, pr) as h:
        out = h.open_eval_batch(X)
        same = []
        for p in range(len(X)):
            one = h.eval(X[p])
            _agrees(_row(out, p), one, f"{name} set {p} vs eval")
            same.append(_bits(_row(out, p), one))
    print(name, dict(same_bits_as_eval=same))          # recorded in DESIGN.md 17, not asserted


# ---- 3. grouping --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d17_J8_L3_K3_sm", "d64_J8_L2_K2_re"])
def test_a_set_does_not_depend_on_groups_neighbours_position_or_P(g, name, monkeypatch):
    pr = tgr.reference_of(name)[0]
    X = _five(pr)
    perm = np.array([3, 0, 4, 2, 1])
    monkeypatch.delenv("GRAPE_OPEN_BATCH_SETS", raising=False)
    with _open(g, pr) as h:
        one = h.open_eval_batch(X)
        info = h.open_batch_info()
        assert info["sets_per_group"] == 5 and info["groups"] == 1
        assert _bits(h.open_eval_batch(X), one)                                  # a repeat call
        moved = h.open_eval_batch(X[perm])
        single = [h.open_eval_batch(X[p:p + 1]) for p in range(5)]
        assert h.open_batch_info()["groups"] == 1 and h.open_batch_info()["sets_per_group"] == 1
    for q, p in enumerate(perm):
        assert _bits(_row(moved, q), _row(one, p)), (q, p)
    for p in range(5):
        assert _bits(_row(single[p], 0), _row(one, p)), p
    monkeypatch.setenv("GRAPE_OPEN_BATCH_SETS", "2")
    with _open(g, pr) as h:
        three = h.open_eval_batch(X)
        info = h.open_batch_info()
        assert info["sets_per_group"] == 2 and info["groups"] == 3
        moved3 = h.open_eval_batch(X[perm])
        assert _bits(h.open_eval_batch(X), three)
        assert h.open_eval_batch(X[:1])[0].shape == (1,) and h.open_batch_info()["groups"] == 1
    assert _bits(three, one)
    assert _bits(moved3, moved)


# ---- 4. more workgroups than CUs -----------------------------------------------------------------------------------------------
def test_more_workgroups_than_compute_units(g):
    """K L P = 360 backward workgroups on 256 CUs: no workgroup waits for another"""
    pr, X, want0, want39 = tbr.many_sets_case()
    oh.assert_order_one(want0)
    oh.assert_order_one(want39)
    with _open(g, pr) as h:
        out = h.open_eval_batch(X)
        info = h.open_batch_info()
        assert info["sets_per_group"] == 40 and info["groups"] == 1
        for p in range(40):
            J, G, tau = h.eval(X[p])
            assert abs(out[0][p] - J) <= TOL_J and np.abs(out[2][p] - tau).max() <= TOL_TAU, p
            assert np.abs(out[1][p] - G).max() <= tol_G(G), p
    _agrees(_row(out, 0), (want0["J"], want0["G"], want0["tau"]), "set 0")
    _agrees(_row(out, 39), (want39["J"], want39["G"], want39["tau"]), "set 39")


# ---- 5. forward only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d17_J8_L3_K3_sm", "d48_J8_L1_K1_re"])
def test_forward_only(g, name):
    pr = tgr.reference_of(name)[0]
    X = _five(pr)
    with _open(g, pr) as h:
        J, G, tau = h.open_eval_batch(X)
        full = h.open_batch_info()
        J0, G0, tau0 = h.open_eval_batch(X, gradient=False)
        info = h.open_batch_info()
    assert G0 is None and np.array_equal(J0, J) and np.array_equal(tau0, tau)
    assert info["terms_backward"] == 0 and full["terms_backward"] > 0
    assert info["terms_forward"] == full["terms_forward"] > 0


# ---- 6. the call disturbs nothing ------------------------------------------------------------------------------------------------
def _record(h, v):
    t = h.timings()
    return dict(tau_grads=h.tau_grads(), storage=h.storage(0), time_gradient=h.time_gradient(), hvp=h.open_hvp(v),
                work=np.array(sorted((k, float(x)) for k, x in h.work().items()), dtype=object).tolist(),
                timings=np.array(sorted((k, float(x)) for k, x in t.items()), dtype=object).tolist(), sums=np.asarray(h.sums()))


def _same_record(a, b):
    return {k: (np.array_equal(np.asarray(a[k]), np.asarray(b[k])) if not isinstance(a[k], list) else a[k] == b[k]) for k in a}


@pytest.mark.parametrize("name", ["d17_J8_L3_K3_sm", "d33_J7_L5_K2_ss"])
def test_the_last_ordinary_evaluation_stays_defined(g, name):
    pr = tgr.reference_of(name)[0]
    x, X = pr["pulsevals"], _five(pr)[1:]
    v = np.cos(np.arange(x.size))
    rng = np.random.default_rng(17)
    t2 = np.concatenate([[0.0], np.cumsum(rng.uniform(0.4, 1.6, 3))])
    with _open(g, pr) as h:
        first = h.eval(x)
        before = _record(h, v)
        out = h.open_eval_batch(X)
        after = _record(h, v)
        assert all(_same_record(before, after).values()), _same_record(before, after)
        again = h.eval(x)
        assert _bits(again, first)
        h.set_tlist(t2)
        moved = h.open_eval_batch(X)
    with _open(g, dict(pr, tlist=t2)) as h:
        fresh = h.open_eval_batch(X)
    assert _bits(moved, fresh)
    assert not np.array_equal(moved[0], out[0])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason_and_leave_the_handle_usable(g):
    pr = tgr.reference_of("d17_J8_L3_K3_sm")[0]
    x = pr["pulsevals"]
    X = _five(pr)
    Jb, taub = np.zeros(5), np.zeros((5, 3), complex)
    with _open(g, pr) as h:
        lib = h._lib
        assert lib.grape_open_eval_batch(None, 5, X.ctypes.data, Jb.ctypes.data, None, None) == -1
        assert lib.grape_last_error(None) == b"grape_open_eval_batch: h == NULL"
        first = h.eval(x)
        firstb = h.open_eval_batch(X)
        for P, px, pj, needle in ((0, X.ctypes.data, Jb.ctypes.data, b"P must be positive"), (-3, X.ctypes.data, Jb.ctypes.data, b"P must be positive"),
                                  (5, None, Jb.ctypes.data, b"pulsevals == NULL"), (5, X.ctypes.data, None, b"J == NULL")):
            assert lib.grape_open_eval_batch(h._h, P, px, pj, None, taub.ctypes.data) == -1
            msg = lib.grape_last_error(h._h)
            assert msg.startswith(b"grape_open_eval_batch: ") and needle in msg, msg
            assert _bits(h.eval(x), first) and _bits(h.open_eval_batch(X), firstb), needle
    # a closed handle
    from grape_jl_amd import synth
    cl = synth.make_problem(5, 2, 3, 2, seed=77)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"], None) as hc:
        firstc = hc.eval(cl["pulsevals"])
        Xc = np.ascontiguousarray(np.stack([cl["pulsevals"], 0.5 * cl["pulsevals"]]))
        assert hc._lib.grape_open_eval_batch(hc._h, 2, Xc.ctypes.data, Jb.ctypes.data, None, None) == -1
        msg = hc._lib.grape_last_error(hc._h)
        assert b"not an open-system handle" in msg and b"use grape_eval_batch" in msg, msg
        info = np.zeros(7)
        assert hc._lib.grape_get_open_batch_info(hc._h, info.ctypes.data, 7) == -1
        assert _bits(hc.eval(cl["pulsevals"]), firstc)
    # a split-phase shard
    sub = dict(pr, H0=pr["H0"][:2], rho0=pr["rho0"][:2], target=pr["target"][:2], weights=pr["weights"][:2])
    with _open(g, sub, K_total=3) as h:
        tau1 = h.forward(x)
        with pytest.raises(g.GrapeHipError, match=r"grape_open_eval_batch: a split-phase shard \(K < K_total\)") as err:
            h.open_eval_batch(X)
        assert err.value.code == -1
        assert np.array_equal(h.forward(x), tau1)
    # a handle without targets
    with _open(g, dict(pr, target=None)) as h:
        tau1 = h.forward(x)
        with pytest.raises(g.GrapeHipError, match=r"grape_open_eval_batch: this handle has no target states") as err:
            h.open_eval_batch(X)
        assert err.value.code == -1
        assert np.array_equal(h.forward(x), tau1)


# ---- 8. defined errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [17, 64])
def test_a_hopeless_set_is_an_error_of_that_set_and_the_handle_recovers(g, d):
    """One set with pulses so large that beta dt > 4096 theta 30 (the GRAPE_ERR_TAYLOR condition of
    test_gpu_open_reference.test_a_hopeless_interval_is_an_error_and_the_handle_recovers, reached through the pulses): the sub-step
    count is clamped, the first series runs into the 200-term limit and every later one is cut after one term.  The call returns
    the status, the message names the set, and the next call gives the bits of the call that never saw the bad set."""
    from grape_jl_amd import synth
    pr = synth.make_open_problem(d, 2, 3, 2, 2, seed=900 + d)
    pr["functional"] = SM
    x = pr["pulsevals"]
    X = np.ascontiguousarray(np.stack([x, 0.5 * x, x[::-1], 1.3 * x]))
    bad = X.copy()
    bad[2] = 1e9 * x       # beta >= 2 sum_l |eps_l| r_l: far above 4096 * 30 * theta / dt
    assert np.abs(bad[2]).max() >= 1e7
    with _open(g, pr) as h:
        first = h.open_eval_batch(X)
        with pytest.raises(g.GrapeHipError) as err:
            h.open_eval_batch(bad)
        assert err.value.code == -5                                 # GRAPE_ERR_TAYLOR
        assert "pulse set 2: " in str(err.value) and "did not converge" in str(err.value)
        again = h.open_eval_batch(X)
        one = h.eval(x)
        h.check()
    assert _bits(again, first)
    _agrees(_row(again, 0), one, "after the error")


@pytest.mark.parametrize("d", [5, 40])
def test_a_zero_weight_under_ss_gives_the_status_of_the_closed_path(g, d):
    """weights = [0, 1] under J_T_ss: chi_0(T) = 0 in every set.  The status is the closed path's, the message names set 0, and
    the forward half stays usable."""
    from grape_jl_amd import synth
    w = np.array([0.0, 1.0])
    cl = synth.make_problem(5, 2, 3, 2, seed=77)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"], w, functional=SS) as hc:
        try:
            hc.eval(cl["pulsevals"])
            rc_closed = 0
        except g.GrapeHipError as e:
            rc_closed = e.code
    pr = synth.make_open_problem(d, 2, 3, 2, 2, seed=910 + d)
    pr["functional"], pr["weights"] = SS, w
    oh.order_one_states(pr, 910 + d)
    x = pr["pulsevals"]
    X = np.ascontiguousarray(np.stack([x, 0.5 * x, 1.3 * x]))
    want = orf.evaluate(pr, X[1], functional=SS)
    with _open(g, pr) as h:
        try:
            h.open_eval_batch(X)
            rc_open = 0
        except g.GrapeHipError as e:
            rc_open = e.code
            assert "pulse set 0: " in str(e) and "chi_min_norm" in str(e)
        print(dict(closed=rc_closed, open=rc_open))
        assert rc_open == rc_closed
        assert rc_open in (0, -3)                                   # GRAPE_ERR_CHI_NORM
        J, _, tau = h.open_eval_batch(X, gradient=False)
    assert abs(J[1] - want["J"]) <= TOL_J and np.abs(tau[1] - want["tau"]).max() <= TOL_TAU
