"""grape_open_hvp: exact Hessian-vector products on open-system handles (csrc/grape_lindblad_hvp.hip.h) -- needs an MI355X.

Against the forward-over-forward reference of tests/open_hvp_reference.py (proved by tests/test_open_hvp_reference.py) on every
NP = 16 / 32 / 48 / 64 instantiation, every functional on every NP, J = 0 ... 8; against the closed path of this library (the
vectorised route through liouvillian(), and pure states at d = 64); against central differences of the device's own G; grouping,
symmetry, a zero direction, route independence, non-interference, every refusal, GRAPE_ERR_TAYLOR, and a Newton-type optimiser.

The comparison with a reference is open_hvp_reference.assert_open_hvp_agrees:
    ||d(Hv)||_inf <= 1e-10 max(||Hv||_inf, 1e-3)                    (the project's tol_hv)
after asserting ON THE REFERENCE ALONE min_k |tau_k| >= 0.1, ||G||_inf >= 1e-3, ||Hv||_inf >= 1e-3: the bound is relative, never its floor.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hvp_reference as hr  # noqa: E402
import open_helpers as oh  # noqa: E402
import open_hvp_reference as ohr  # noqa: E402
from open_hvp_reference import RE, SM, SS  # noqa: E402

pytestmark = pytest.mark.gpu

THETA = 3.0   # sub-step threshold of the kernels


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


# name -> case spec of open_time_reference.build_case (N_T = 3) plus nv and zero_interval (open_hvp_reference.reference_of).
# Eight collapse operators mix the state quickly: where the target of the pulse 0.8 x left the signals small the case takes the
# target of the pulse -0.8 x.
GRID = dict(weights=True, shape=True, nonuniform=True)
CASES = {
    "d4_J2_L2_sm": dict(d=4, J=2, L=2, K=2, functional=SM, nonuniform=True, nv=3),
    "d12_J8_L3_ss": dict(d=12, J=8, L=3, K=2, functional=SS, nonuniform=True),
    "d16_J1_L2_re": dict(d=16, J=1, L=2, K=2, functional=RE, nonuniform=True),
    "d17_J8_L3_K3_sm": dict(d=17, J=8, L=3, K=3, functional=SM, factor=-0.8, zero_interval=1, **GRID),
    "d31_J1_L1_re": dict(d=31, J=1, L=1, K=2, functional=RE, hermitian=False, non_hermitian_states=0.3, nonuniform=True),
    "d32_J4_L2_ss": dict(d=32, J=4, L=2, K=2, functional=SS, cops_per_traj=True, nonuniform=True),
    "d33_J7_L5_re": dict(d=33, J=7, L=5, K=2, functional=RE, nonuniform=True, nv=1),
    "d47_J0_L2_sm": dict(d=47, J=0, L=2, K=2, functional=SM, hc_per_traj=True, nonuniform=True, nv=1),
    "d49_J5_L2_ss": dict(d=49, J=5, L=2, K=2, functional=SS, weights=True, nonuniform=True, nv=1),
    "d63_J2_L2_re": dict(d=63, J=2, L=2, K=2, functional=RE, hermitian=False, non_hermitian_states=0.3,
                         non_hermitian_controls=True, nonuniform=True, nv=1),
    "d64_J8_L2_K2_sm": dict(d=64, J=8, L=2, K=2, functional=SM, factor=-0.8, nv=1, **GRID),
    # further checks (not rows of the table)
    "d20_J2": dict(d=20, J=2, L=2, K=2, functional=SM, nv=2, **GRID),
    "d5_J2": dict(d=5, J=2, L=2, K=2, functional=SM, nv=5, **GRID),
}
TABLE = [name for name in CASES if name not in ("d20_J2", "d5_J2")]


def _open(g, pr, functional=None, **kw):
    return g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr.get("target"), pr.get("weights"),
                          functional=pr["functional"] if functional is None else functional, shape=pr.get("shape"), **kw)


def _tlist(dts):
    return np.concatenate([[0.0], np.cumsum(dts)])


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE)
def test_against_the_forward_over_forward_reference(g, name):
    pr, V, want = ohr.reference_of(name, CASES)
    with _open(g, pr) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        got = h.open_hvp(V)
        info = h.open_hvp_info()
    assert abs(J - want["J"]) <= oh.TOL_J and np.abs(tau - want["tau"]).max() <= oh.TOL_TAU
    assert np.abs(G - want["G"]).max() <= oh.tol_G(want["G"])
    ohr.assert_open_hvp_agrees(got, want, name)
    K, L, N_T, nv = pr["H0"].shape[0], np.asarray(pr["Hc"]).shape[-3], 3, len(V)
    assert info["series_steps"] >= nv * (K + K * L) * N_T and info["dirs_per_group"] == nv
    assert info["series_terms"] == info["terms_forward"] + info["terms_backward"] > 0 and info["bytes"] > 0


def _kernel_beta(pr, k, n):
    """beta_n of the kernels' sub-step rule, up to their norm estimate: 1.1 x a power-iteration value that
    lies a few per cent below the 2-norm at most"""
    n2 = lambda A: np.linalg.norm(A, 2)   # noqa: E731
    L, N_T = pr["Hc"].shape[0], len(pr["tlist"]) - 1
    e = np.abs(pr["pulsevals"].reshape(L, N_T)[:, n])
    return 1.1 * (2.0 * (n2(pr["H0"][k]) + sum(e[l] * n2(pr["Hc"][l]) for l in range(L)))) + 1.21 * sum(n2(A) ** 2 for A in pr["cops"])


def test_d48_one_interval_of_three_substeps(g):
    """d = 48, J = 8, L = 1, K = 1, J_T_ss: interval 1 has beta dt / theta just above 2 (2.25, with the 5 % the norm estimate may lie
    lower: three sub-steps), the outer ones one sub-step each; the count is asserted from the info call"""
    from grape_jl_amd import synth
    d, L, K, N_T, nv = 48, 1, 1, 3, 2
    pr = synth.make_open_problem(d, L, N_T, K, 8, seed=4808)
    beta = _kernel_beta(pr, 0, 1)
    dt1, dt0 = 2.25 * THETA / beta, 0.3 * THETA / beta
    assert 2 < 0.95 * beta * dt1 / THETA and beta * dt1 / THETA < 3
    pr["tlist"] = _tlist([dt0, dt1, dt0])
    pr["functional"] = SS
    oh.order_one_states(pr, 4808, factor=-0.8)
    x = pr["pulsevals"]
    V = ohr.directions(4808, nv, x.size)
    want = ohr.evaluate(pr, x, V, SS)
    with _open(g, pr) as h:
        h.eval(x)
        got = h.open_hvp(V)
        info = h.open_hvp_info()
    ohr.assert_open_hvp_agrees(got, want, "d48, three sub-steps")
    assert info["series_steps"] == nv * (K + K * L) * (1 + 3 + 1)


# ---- 2. against the closed path of this library -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 8])
def test_vectorised_route_of_the_same_library(g, d):
    """GrapeHip.hvp on liouvillian(): N = 16 and N = 64, the largest the closed grape_hvp takes"""
    import open_time_reference as otr
    pr = otr.build_case(dict(d=d, J=2, L=2, K=2, functional=SM, **GRID))
    K, L = 2, 2
    x = pr["pulsevals"]
    V = ohr.directions(40 + d, 2, x.size)
    Hv = np.stack([g.liouvillian(pr["H0"][k], pr["cops"]) for k in range(K)])
    Hcv = np.stack([g.liouvillian(pr["Hc"][l]) for l in range(L)])
    with g.GrapeHip(Hv, Hcv, pr["tlist"], oh.vec(pr["rho0"]), oh.vec(pr["target"]), pr["weights"], functional=SM,
                    shape=pr["shape"]) as hv:
        Jv, Gv, tauv = hv.eval(x)
        want = hv.hvp(V)
    with _open(g, pr) as h:
        J, G, tau = h.eval(x)
        got = h.open_hvp(V)
    size = float(np.abs(want).max())
    print(dict(d=d, dev=float(np.abs(got - want).max()), size=size))
    assert abs(J - Jv) <= oh.TOL_J and np.abs(tau - tauv).max() <= oh.TOL_TAU
    assert np.abs(tauv).min() >= 0.1 and size >= 1e-3
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, size)


def test_pure_states_at_d64_against_the_closed_path(g):
    """J = 0, rho(0) = |psi><psi|, sigma = |tgt><tgt|: tau_open = |tau_closed|^2, so J_T_re here is J_T_ss there"""
    import scipy.linalg
    from grape_jl_amd import synth
    d, L, N_T, K = 64, 2, 3, 2
    cl = synth.make_problem(d, L, N_T, K, seed=6400)
    rng = np.random.default_rng(6400)
    tl = _tlist(rng.uniform(0.5, 1.5, N_T))
    w = np.array([0.5, 1.5])
    x = cl["pulsevals"]
    V = ohr.directions(6400, 2, x.size)
    tgt = cl["psi0"].copy()        # the state the pulse 0.8 x reaches: tau = O(1)
    for k in range(K):
        for n in range(N_T):
            H = cl["H0"][k] + sum(0.8 * x[l * N_T + n] * cl["Hc"][l] for l in range(L))
            tgt[k] = scipy.linalg.expm(-1j * H * (tl[n + 1] - tl[n])) @ tgt[k]
    with g.GrapeHip(cl["H0"], cl["Hc"], tl, cl["psi0"], tgt, w, functional=g.J_T_SS) as hc:
        Jc, Gc, tauc = hc.eval(x)
        want = hc.hvp(V)
    proj = lambda v: v[:, :, None] * v[:, None, :].conj()   # noqa: E731
    op = dict(H0=cl["H0"], Hc=cl["Hc"], cops=None, tlist=tl, rho0=proj(cl["psi0"]), target=proj(tgt), weights=w, functional=RE)
    with _open(g, op) as h:
        J, G, tau = h.eval(x)
        got = h.open_hvp(V)
    assert abs(J - Jc) <= oh.TOL_J and np.abs(tau - np.abs(tauc) ** 2).max() <= oh.TOL_TAU
    assert np.abs(tauc).min() ** 2 >= 0.1 and np.abs(Gc).max() >= 1e-3 and np.abs(want).max() >= 1e-3
    hr.assert_hvp_agrees(got, want, "pure d64")


# ---- 3. without a reference: central differences of the device's own G ----------------------------------------------------------
def test_against_central_differences_of_the_devices_G(g):
    """4th-order central differences, h = 1e-3: truncation h^4 G^(5) / 30 ~ 3e-14, rounding of G (1e-15) / h ~ 1e-12, against
    ||Hv||_inf ~ 1e-1: the relative bound 1e-6 leaves four digits"""
    pr, V, want = ohr.reference_of("d20_J2", CASES)
    x, hs = pr["pulsevals"], 1e-3
    with _open(g, pr) as h:
        h.eval(x)
        got = h.open_hvp(V)
        fd = np.stack([(-h.eval(x + 2 * hs * v)[1] + 8 * h.eval(x + hs * v)[1] - 8 * h.eval(x - hs * v)[1] + h.eval(x - 2 * hs * v)[1]) / (12 * hs)
                       for v in V])
    size = float(np.abs(got).max())
    print(dict(dev=float(np.abs(got - fd).max()), size=size))
    assert size >= 1e-3
    assert np.abs(got - fd).max() <= 1e-6 * size
    ohr.assert_open_hvp_agrees(got, want, "d20")


# ---- 4. grouping, symmetry, routes ------------------------------------------------------------------------------------------
def test_grouping_never_changes_a_direction(g, monkeypatch):
    """nv = 5 in one call against five calls, and against launch groups of two (GRAPE_HVP_DIRS=2, read at create): bit for bit"""
    pr, V, want = ohr.reference_of("d5_J2", CASES)
    x = pr["pulsevals"]
    with _open(g, pr) as h:
        h.eval(x)
        together = h.open_hvp(V)
        assert h.open_hvp_info()["dirs_per_group"] == 5
        bytes5 = h.open_hvp_info()["bytes"]
        single = np.stack([h.open_hvp(v) for v in V])
        assert h.open_hvp_info()["dirs_per_group"] == 1 and h.open_hvp_info()["bytes"] == bytes5       # (the storage only grows)
        again = h.open_hvp(V)
    monkeypatch.setenv("GRAPE_HVP_DIRS", "2")
    with _open(g, pr) as h:
        h.eval(x)
        grouped = h.open_hvp(V)
        info = h.open_hvp_info()
    monkeypatch.delenv("GRAPE_HVP_DIRS")
    assert info["dirs_per_group"] == 2 and 0 < info["bytes"] < bytes5
    assert np.array_equal(together, single) and np.array_equal(together, again) and np.array_equal(together, grouped)
    ohr.assert_open_hvp_agrees(together, want, "d5, five directions")
    # the Hessian is symmetric: v_i . H v_j = v_j . H v_i on the device
    A = V @ together.T
    scale = float(np.abs(A).max())
    print(dict(asym=float(np.abs(A - A.T).max()), scale=scale))
    assert scale >= 1e-3 and np.abs(A - A.T).max() <= 1e-10 * scale


def test_a_direction_that_is_zero_on_one_interval(g):
    """v_n = 0 on interval 1: B = 0 there, the tangent chain has a zero source, and before any non-zero interval (sweeping
    backwards under J_T_re, chi' = 0) whole chains are identically zero -- they count as converged"""
    pr, V, want = ohr.reference_of("d16_J1_L2_re", CASES)
    x = pr["pulsevals"]
    Vz = V.reshape(len(V), 2, 3).copy()
    Vz[0, :, 1] = 0.0
    Vz[1, :, 2] = 0.0      # the last interval: the first of the backward sweep
    Vz = Vz.reshape(len(V), -1)
    key = "zero_d16"
    if key not in ohr._CACHE:
        ohr._CACHE[key] = ohr.evaluate(pr, x, Vz, RE)
    with _open(g, pr) as h:
        h.eval(x)
        got = h.open_hvp(Vz)
        zero = h.open_hvp(np.zeros_like(x))
    ohr.assert_open_hvp_agrees(got, ohr._CACHE[key], "zero intervals")
    assert np.array_equal(zero, np.zeros_like(x))


def test_every_route_to_a_forward_state_gives_the_same_bits(g):
    pr, V, want = ohr.reference_of("d17_J8_L3_K3_sm", CASES)
    x = pr["pulsevals"]
    with _open(g, pr) as h:
        h.eval(x)
        full = h.open_hvp(V)
        h.eval(x, gradient=False)
        no_gradient = h.open_hvp(V)
        h.forward(x)
        forward_only = h.open_hvp(V)
        h.backward(complex(*h.sums()[:2]))
        both_halves = h.open_hvp(V)
    assert np.array_equal(full, no_gradient) and np.array_equal(full, forward_only) and np.array_equal(full, both_halves)


# ---- 5. non-interference --------------------------------------------------------------------------------------------------------
def test_the_call_disturbs_nothing_and_repeats_bitwise(g):
    pr, V, want = ohr.reference_of("d33_J7_L5_re", CASES)
    x = pr["pulsevals"]
    with _open(g, pr) as h:
        J, G, tau = h.eval(x)
        before = dict(tg=h.tau_grads(), work=h.work(), timings=h.timings(), store=h.storage(0), dJdt=h.time_gradient())
        a = h.open_hvp(V)
        b = h.open_hvp(V)
        after = dict(tg=h.tau_grads(), work=h.work(), timings=h.timings(), store=h.storage(0), dJdt=h.time_gradient())
        assert np.array_equal(a, b)
        assert np.array_equal(before["tg"], after["tg"]) and np.array_equal(before["store"], after["store"])
        assert np.array_equal(before["dJdt"], after["dJdt"])
        assert before["work"] == after["work"] and before["timings"] == after["timings"]
        assert before["timings"]["forward"] > 0.0 and before["work"]["series_terms"] > 0
        J1, G1, tau1 = h.eval(x)
        assert J1 == J and np.array_equal(G1, G) and np.array_equal(tau1, tau)
        assert np.array_equal(h.tau_grads(), before["tg"]) and np.array_equal(h.time_gradient(), before["dJdt"])
        assert np.array_equal(h.open_hvp(V), a)
    ohr.assert_open_hvp_agrees(a, want, "d33")


# ---- 6. refusals and errors ---------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason_and_leave_the_handle_usable(g):
    from grape_jl_amd import synth
    pr, V, want = ohr.reference_of("d5_J2", CASES)
    x = pr["pulsevals"]
    v = np.ascontiguousarray(V[0])
    out = np.zeros_like(v)
    pv, po = v.ctypes.data, out.ctypes.data
    with _open(g, pr) as h:
        lib, hd = h._lib, h._h

        def refused(needle, call=lambda: lib.grape_open_hvp(hd, 1, pv, po), handle=hd):
            assert call() == -1, needle
            msg = lib.grape_last_error(handle)
            assert b"grape_open_hvp" in msg and needle in msg, (needle, msg)

        refused(b"no evaluation")
        first = h.eval(x)
        tg = h.tau_grads()
        hv = h.open_hvp(V)

        def same_bits():
            J, G, tau = h.eval(x)
            assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(tau, first[2])
            assert np.array_equal(h.tau_grads(), tg) and np.array_equal(h.open_hvp(V), hv)

        refused(b"h == NULL", lambda: lib.grape_open_hvp(None, 1, pv, po), None)
        same_bits()
        for call in (lambda: lib.grape_open_hvp(hd, 0, pv, po), lambda: lib.grape_open_hvp(hd, -3, pv, po),
                     lambda: lib.grape_open_hvp(hd, 1, None, po), lambda: lib.grape_open_hvp(hd, 1, pv, None)):
            refused(b"nv must be positive, V and HV must not be NULL", call)
            same_bits()
        h.set_tlist(pr["tlist"])
        refused(b"grape_set_tlist")
        same_bits()
        h.eval_batch(np.stack([x, 0.5 * x]))
        refused(b"grape_eval_batch")
        same_bits()
        bad = pr["tlist"].copy()
        bad[2:] += 1e6 - 1.0         # a hopeless interval: GRAPE_ERR_TAYLOR from the evaluation (test_gpu_open_reference.py)
        h.set_tlist(bad)
        with pytest.raises(g.GrapeHipError) as err:
            h.eval(x)
        assert err.value.code == -5
        refused(b"failed")
        h.set_tlist(pr["tlist"])
        same_bits()
        with pytest.raises(g.GrapeHipError) as err:      # the Python method raises what the library says
            h.set_tlist(pr["tlist"])
            h.open_hvp(V)
        assert err.value.code == -1 and "grape_set_tlist" in str(err.value)
        same_bits()
        h.check()
    # a split-phase shard, and a handle without targets
    with _open(g, dict(pr, H0=pr["H0"][:1], rho0=pr["rho0"][:1], target=pr["target"][:1], weights=pr["weights"][:1]), K_total=2) as hs:
        hs.forward(x)
        assert hs._lib.grape_open_hvp(hs._h, 1, pv, po) == -1
        assert b"K < K_total" in hs._lib.grape_last_error(hs._h)
        hs.backward(complex(*hs.sums()[:2]))
    with _open(g, dict(pr, target=None)) as hn:
        hn.forward(x)
        assert hn._lib.grape_open_hvp(hn._h, 1, pv, po) == -1
        assert b"no target states" in hn._lib.grape_last_error(hn._h)
        hn.forward(x)
    # a closed handle: the message names grape_hvp, and grape_hvp on an open handle names this call
    cl = synth.make_problem(5, 2, 3, 2, seed=77)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"]) as hc:
        Jc, Gc, _ = hc.eval(cl["pulsevals"])
        assert hc._lib.grape_open_hvp(hc._h, 1, pv, po) == -1
        msg = hc._lib.grape_last_error(hc._h)
        assert b"grape_hvp" in msg and b"not an open-system handle" in msg
        assert hc._lib.grape_get_open_hvp_info(hc._h, po, 7) == -1
        J2, G2, _ = hc.eval(cl["pulsevals"])
        assert J2 == Jc and np.array_equal(G2, Gc)
    with _open(g, pr) as h:
        h.eval(x)
        assert h._lib.grape_hvp(h._h, 1, pv, po) == -1
        msg = h._lib.grape_last_error(h._h)
        assert b"open-system" in msg and b"grape_open_hvp" in msg
        assert np.array_equal(h.open_hvp(V), hv)


def test_a_series_that_cannot_converge_is_grape_err_taylor(g):
    """The over-long interval of tests/test_gpu_open_reference.py stops the EVALUATION with GRAPE_ERR_TAYLOR, so this call refuses
    (no valid forward state).  Its own GRAPE_ERR_TAYLOR needs a valid forward state and a series that cannot converge: a
    direction that is not finite (every norm is NaN, no stopping rule holds, the first series runs into the 200-term limit and
    every later one is cut after one term).  Back on finite input the handle gives its first result bit for bit."""
    pr, V, want = ohr.reference_of("d5_J2", CASES)
    x = pr["pulsevals"]
    bad = pr["tlist"].copy()
    bad[2:] += 1e6 - 1.0
    with _open(g, pr) as h:
        first = h.eval(x)
        hv = h.open_hvp(V)
        h.set_tlist(bad)
        with pytest.raises(g.GrapeHipError) as err:
            h.eval(x)
        assert err.value.code == -5
        with pytest.raises(g.GrapeHipError) as err:
            h.open_hvp(V)
        assert err.value.code == -1 and "failed" in str(err.value)
        h.set_tlist(pr["tlist"])                       # the sane grid again
        J, G, tau = h.eval(x)
        assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(h.open_hvp(V), hv)
        Vn = V.copy()
        Vn[1, 0] = np.nan
        with pytest.raises(g.GrapeHipError) as err:
            h.open_hvp(Vn)
        assert err.value.code == -5 and "did not converge" in str(err.value)
        assert np.array_equal(h.open_hvp(V), hv)            # ... without a new evaluation: the forward state is still valid
        J, G, tau = h.eval(x)
        assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(tau, first[2])
        h.check()


# ---- 7. the optimiser the call is for -------------------------------------------------------------------------------------------
def test_trust_ncg_drives_a_dissipative_state_transfer(g):
    """d = 3 ladder with amplitude damping, |0><0| -> |1><1| under J_T_re: scipy's trust-ncg with hessp = GrapeHipOpen.open_hvp
    reaches a J no higher than L-BFGS-B from the same start"""
    import scipy.optimize
    d, N_T, T = 3, 6, 4.0
    a = np.diag(np.sqrt(np.arange(1.0, d)), 1).astype(complex)
    H0 = np.diag([0.0, 0.0, -0.6]).astype(complex)[None]
    Hc = np.stack([0.5 * (a + a.conj().T), 0.5j * (a - a.conj().T)])
    cops = np.sqrt(0.02) * a[None]
    rho0 = np.zeros((1, d, d), complex)
    rho0[0, 0, 0] = 1.0
    target = np.zeros((1, d, d), complex)
    target[0, 1, 1] = 1.0
    t = (np.arange(N_T) + 0.5) / N_T
    x0 = np.concatenate([0.4 * np.sin(np.pi * t), 0.1 * np.cos(np.pi * t)])
    with g.GrapeHipOpen(H0, Hc, cops, np.linspace(0.0, T, N_T + 1), rho0, target, functional=RE) as h:

        at = [None]

        def fg(x):
            J, G, _ = h.eval(x)
            at[0] = x.copy()
            return J, G.copy()

        def hessp(x, p):
            if not np.array_equal(x, at[0]):      # (after a rejected trial step the handle holds the trial point's states)
                h.eval(x, gradient=False)
                at[0] = x.copy()
            return h.open_hvp(p)

        J0 = fg(x0)[0]
        lb = scipy.optimize.minimize(fg, x0, jac=True, method="L-BFGS-B")
        nc = scipy.optimize.minimize(fg, x0, jac=True, hessp=hessp, method="trust-ncg", options=dict(gtol=1e-9, maxiter=200))
    print(dict(J0=J0, lbfgs=lb.fun, nit_lbfgs=lb.nit, trust_ncg=nc.fun, nit_ncg=nc.nit, nhev=nc.nhev))
    assert lb.fun < 0.5 * J0                      # a real descent, to a decoherence-limited optimum (J > 0)
    assert nc.fun > 0.0
    assert nc.fun <= lb.fun
