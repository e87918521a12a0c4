"""grape_open_time_gradient: dJ/d dt_n on open-system handles (csrc/grape_lindblad_tg.hip.h) -- needs an MI355X.

Against the forward-sensitivity reference of tests/open_time_reference.py (proved by tests/test_open_time_reference.py) on every
NP = 16 / 32 / 48 / 64 instantiation, every functional on every NP, J = 0 ... 8; against central differences of the device's
own J; against the closed path of this library (pure states, and the vectorised route through liouvillian()); an interval
split in two; shards; the caller's chi; the state machine of the entry point; non-interference and repeatability.

The comparison with a reference is open_time_reference.assert_time_gradient_agrees:
    ||d(dJ/d dt)||_inf <= 1e-10 max(||dJ/d dt||_inf, 1e-3)         (the project's tol_G rule)
after asserting ON THE REFERENCE ALONE ||dJ/d dt||_inf >= 1e-3 and min_k |tau_k| >= 0.1: the bound is relative, never its floor.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
import open_time_reference as otr  # noqa: E402
from open_time_reference import RE, SM, SS  # noqa: E402

pytestmark = pytest.mark.gpu

THETA = 3.0   # sub-step threshold of the kernels


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


# name -> case spec of open_time_reference.build_case (N_T = 3).  Eight collapse operators mix the state quickly: where the
# target of the pulse 0.8 x left the signals small the case takes the target of the pulse -0.8 x.
GRID = dict(weights=True, shape=True, nonuniform=True)
CASES = {
    "d4_J2_L2_sm": dict(d=4, J=2, L=2, K=2, functional=SM, nonuniform=True),
    "d12_J8_L3_ss": dict(d=12, J=8, L=3, K=2, functional=SS, nonuniform=True),
    "d16_J1_L2_re": dict(d=16, J=1, L=2, K=2, functional=RE, nonuniform=True),
    "d17_J8_L3_K3_sm": dict(d=17, J=8, L=3, K=3, functional=SM, factor=-0.8, **GRID),
    "d31_J1_L1_re": dict(d=31, J=1, L=1, K=2, functional=RE, nonuniform=True),
    "d32_J4_L2_ss": dict(d=32, J=4, L=2, K=2, functional=SS, cops_per_traj=True, nonuniform=True),
    "d33_J7_L5_re": dict(d=33, J=7, L=5, K=2, functional=RE, nonuniform=True),
    "d47_J0_L2_sm": dict(d=47, J=0, L=2, K=2, functional=SM, hc_per_traj=True, nonuniform=True),
    "d48_J8_L1_K1_ss": dict(d=48, J=8, L=1, K=1, functional=SS, long_step=6.0, dt=0.5, factor=-0.8),
    "d49_J5_L2_ss": dict(d=49, J=5, L=2, K=2, functional=SS, weights=True, nonuniform=True),
    "d63_J2_L2_re": dict(d=63, J=2, L=2, K=2, functional=RE, hermitian=False, non_hermitian_states=0.3,
                         non_hermitian_controls=True, nonuniform=True),
    "d64_J8_L2_K2_sm": dict(d=64, J=8, L=2, K=2, functional=SM, factor=-0.8, **GRID),
    # further checks (not rows of the table)
    "d20_J2": dict(d=20, J=2, L=2, K=2, functional=SM, **GRID),
    "shards_d48": dict(d=48, J=2, L=2, K=2, functional=SM, **GRID),
}
TABLE = [name for name in CASES if name[0] == "d" and name != "d20_J2"]


def _open(g, pr, functional=None, **kw):
    return g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr.get("target"), pr.get("weights"),
                          functional=pr["functional"] if functional is None else functional, shape=pr.get("shape"), **kw)


def _tlist(dts):
    return np.concatenate([[0.0], np.cumsum(dts)])


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE)
def test_against_the_forward_sensitivity_reference(g, name):
    pr, want = otr.reference_of(name, CASES)
    with _open(g, pr) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        got = h.time_gradient()
        work = h.work()
    assert abs(J - want["J"]) <= oh.TOL_J and np.abs(tau - want["tau"]).max() <= oh.TOL_TAU
    otr.assert_time_gradient_agrees(got, want["dJdt"], want["tau"], name)
    N_T, K = len(pr["tlist"]) - 1, pr["H0"].shape[0]
    if CASES[name].get("long_step"):      # the long interval was cut into sub-steps (forward sweep + chi chain of the evaluation)
        assert work["series_steps"] > 2 * K * N_T
    else:
        assert work["series_steps"] >= 2 * K * N_T


# ---- 2. without the reference: central differences of the device's own J -------------------------------------------------------
def test_against_central_differences_of_the_devices_J(g):
    """4th-order central differences, h = 1e-4: truncation h^4 J^(5) / 30 ~ 1e-17, rounding of J (1e-15) / h ~ 1e-11, against
    ||dJ/d dt||_inf ~ 1e-2: the relative bound 1e-6 leaves three digits.  The same for the duration of a scaled grid."""
    pr, want = otr.reference_of("d20_J2", CASES)
    x, hstep = pr["pulsevals"], 1e-4
    dts = np.diff(pr["tlist"])
    with _open(g, pr) as h:
        h.eval(x)
        got = h.time_gradient()

        def Jat(q):
            h.set_tlist(_tlist(q))
            return h.eval(x, gradient=False)[0]

        fd = np.empty(len(dts))
        for n in range(len(dts)):
            e = np.zeros(len(dts))
            e[n] = hstep
            fd[n] = (-Jat(dts + 2 * e) + 8 * Jat(dts + e) - 8 * Jat(dts - e) + Jat(dts - 2 * e)) / (12 * hstep)
        # dJ/dT on the scaled grid dt_n -> (1 + s) dt_n: dJ/ds = T dJ/dT = sum_n dt_n dJ/d dt_n
        fs = (-Jat(dts * (1 + 2 * hstep)) + 8 * Jat(dts * (1 + hstep)) - 8 * Jat(dts * (1 - hstep)) + Jat(dts * (1 - 2 * hstep))) / (12 * hstep)
    T = dts.sum()
    size = np.abs(got).max()
    print(dict(dev=np.abs(got - fd).max(), size=size, dJdT=np.sum(dts / T * got), dJdT_fd=fs / T))
    assert size >= 1e-3
    assert np.abs(got - fd).max() <= 1e-6 * size
    assert abs(np.sum(dts / T * got) - fs / T) <= 1e-6 * size
    otr.assert_time_gradient_agrees(got, want["dJdt"], want["tau"], "d20")


# ---- 3. against the closed path of this library -------------------------------------------------------------------------------
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
    tgt = cl["psi0"].copy()        # the state the pulse 0.8 x reaches: tau = O(1)
    for k in range(K):
        for n in range(N_T):
            H = cl["H0"][k] + sum(0.8 * x[l * N_T + n] * cl["Hc"][l] for l in range(L))
            tgt[k] = scipy.linalg.expm(-1j * H * (tl[n + 1] - tl[n])) @ tgt[k]
    with g.GrapeHip(cl["H0"], cl["Hc"], tl, cl["psi0"], tgt, w, functional=g.J_T_SS) as hc:
        Jc, _, tauc = hc.eval(x)
        want = hc.time_gradient()
    proj = lambda v: v[:, :, None] * v[:, None, :].conj()   # noqa: E731
    op = dict(H0=cl["H0"], Hc=cl["Hc"], cops=None, tlist=tl, rho0=proj(cl["psi0"]), target=proj(tgt), weights=w, functional=RE)
    with _open(g, op) as h:
        J, _, tau = h.eval(x)
        got = h.time_gradient()
    assert abs(J - Jc) <= oh.TOL_J and np.abs(tau - np.abs(tauc) ** 2).max() <= oh.TOL_TAU
    otr.assert_time_gradient_agrees(got, want, np.abs(tauc) ** 2, "pure d64")


@pytest.mark.parametrize("d", [4, 9])
def test_vectorised_route_of_the_same_library(g, d):
    """GrapeHip on liouvillian(): N = 16 (the fused path) and N = 81 (the blocked path)"""
    pr, ref = otr.reference_of(f"vec_d{d}", {f"vec_d{d}": dict(d=d, J=2, L=2, K=2, functional=SM, **GRID)})
    K, L = 2, 2
    Hv = np.stack([g.liouvillian(pr["H0"][k], pr["cops"]) for k in range(K)])
    Hcv = np.stack([g.liouvillian(pr["Hc"][l]) for l in range(L)])
    with g.GrapeHip(Hv, Hcv, pr["tlist"], oh.vec(pr["rho0"]), oh.vec(pr["target"]), pr["weights"], functional=SM,
                    shape=pr["shape"]) as hv:
        Jv, _, tauv = hv.eval(pr["pulsevals"])
        want = hv.time_gradient()
    with _open(g, pr) as h:
        J, _, tau = h.eval(pr["pulsevals"])
        got = h.time_gradient()
    assert abs(J - Jv) <= oh.TOL_J and np.abs(tau - tauv).max() <= oh.TOL_TAU
    otr.assert_time_gradient_agrees(got, want, tauv, f"vectorised d={d}")
    otr.assert_time_gradient_agrees(got, ref["dJdt"], ref["tau"], f"reference d={d}")


# ---- 4. an interval split in two with the same pulses -------------------------------------------------------------------------
def _kernel_beta(pr, k, n):
    """beta_n of the kernels' sub-step rule, up to their norm estimate: 1.1 x a power-iteration value that
    lies a few per cent below the 2-norm at most"""
    n2 = lambda A: np.linalg.norm(A, 2)   # noqa: E731
    L, N_T = pr["Hc"].shape[0], len(pr["tlist"]) - 1
    e = np.abs(pr["pulsevals"].reshape(L, N_T)[:, n])
    return 1.1 * (2.0 * (n2(pr["H0"][k]) + sum(e[l] * n2(pr["Hc"][l]) for l in range(L)))) + 1.21 * sum(n2(A) ** 2 for A in pr["cops"])


@pytest.mark.parametrize("x_whole,sub_whole,sub_halves", [(1.85, 2, 1), (2.25, 3, 2)], ids=["below", "above"])
@pytest.mark.parametrize("d", [20, 64])
def test_splitting_an_interval(g, d, x_whole, sub_whole, sub_halves):
    """Interval 1 replaced by two of half the length with the same pulse value: exp(L dt) commutes with L, so both halves and
    the unsplit interval have the same dJ/d dt, and the other intervals keep theirs -- exact in exact arithmetic, through
    another loop structure on the device (2 sub-steps against 1 + 1, or 3 of dt / 3 against 2 + 2 of dt / 4): 1e-12 relative,
    the tolerance of the route-independence tests of DESIGN.md 14."""
    from grape_jl_amd import synth
    L, K, N_T = 2, 2, 3
    pr = synth.make_open_problem(d, L, N_T, K, 2, seed=700 + d)
    pr["weights"] = np.array([0.7, 1.3])
    x = pr["pulsevals"]
    beta = max(_kernel_beta(pr, k, 1) for k in range(K))
    beta_lo = min(_kernel_beta(pr, k, 1) for k in range(K))
    dt1 = x_whole * THETA / beta
    # both trajectories on the intended side, with the 5 % the norm estimate may lie lower
    assert sub_whole - 1 < 0.95 * beta_lo * dt1 / THETA and beta * dt1 / THETA < sub_whole
    assert sub_halves - 1 < 0.95 * beta_lo * dt1 / (2 * THETA) and beta * dt1 / (2 * THETA) < sub_halves
    dt0 = 0.3 * THETA / beta      # the outer intervals: one sub-step each
    pr["tlist"] = np.array([0.0, dt0, dt0 + dt1, 2 * dt0 + dt1])
    tl_split = np.array([0.0, dt0, dt0 + 0.5 * dt1, dt0 + dt1, 2 * dt0 + dt1])
    x2 = x.reshape(L, N_T)[:, [0, 1, 1, 2]].reshape(-1)
    oh.order_one_states(pr, 700 + d)
    with _open(g, pr, SM) as h:
        _, _, tau = h.eval(x)
        steps = h.work()["series_steps"]
        whole = h.time_gradient()
    with _open(g, dict(pr, tlist=tl_split), SM) as h:
        h.eval(x2)
        steps_split = h.work()["series_steps"]
        split = h.time_gradient()
    assert steps == 2 * K * (2 + sub_whole) and steps_split == 2 * K * (2 + 2 * sub_halves)
    size = np.abs(whole).max()
    dev = np.abs(split - whole[[0, 1, 1, 2]]).max()
    print(dict(d=d, whole=whole, split=split, rel=dev / size))
    assert np.abs(tau).min() >= 0.1 and size >= 1e-3
    assert dev <= 1e-12 * size


# ---- 5. shards ---------------------------------------------------------------------------------------------------------------
def test_two_shards_at_d48(g):
    pr, want = otr.reference_of("shards_d48", CASES)
    x = pr["pulsevals"]
    with _open(g, pr) as h:
        h.eval(x)
        single = h.time_gradient()
    parts = []
    for s in (slice(0, 1), slice(1, 2)):
        sub = dict(pr, H0=pr["H0"][s], rho0=pr["rho0"][s], target=pr["target"][s], weights=pr["weights"][s])
        parts.append(_open(g, sub, K_total=2))
    try:
        for h in parts:
            h.forward(x)
        sums = sum(h.sums() for h in parts)
        f = complex(sums[0], sums[1])
        for h in parts:
            h.backward(f)
        partial = [h.time_gradient() for h in parts]
    finally:
        for h in parts:
            h.close()
    total = partial[0] + partial[1]
    size = np.abs(single).max()
    print(dict(single=single, partial=partial, rel=np.abs(total - single).max() / size))
    assert np.abs(partial[0]).max() > 0 and np.abs(partial[1]).max() > 0
    assert np.abs(total - single).max() <= 1e-12 * size
    otr.assert_time_gradient_agrees(total, want["dJdt"], want["tau"], "shards")


# ---- 6. the caller's chi --------------------------------------------------------------------------------------------------------
def test_backward_chi_at_d33(g):
    import open_reference as orf
    name = "d33_J7_L5_re"
    pr, want = otr.reference_of(name, CASES)
    x, K = pr["pulsevals"], 2
    # a chi of the caller's own: not a multiple of the targets, not Hermitian, O(1) overlaps
    from grape_jl_amd import synth
    z = synth.normal(synth.subseed(33, 1), 2 * K * 33 * 33).reshape(2, K, 33, 33)
    chi = 0.4 * pr["target"] + 0.3 / 33 * (z[0] + 1j * z[1])
    if "chi33" not in otr._CACHE:
        otr._CACHE["chi33"] = otr.time_gradient(pr, x, boundary=chi)
    want_chi = otr._CACHE["chi33"]
    with _open(g, dict(pr, target=None)) as h:       # a handle without targets: chi can only be the caller's
        h.forward(x)
        h.backward_chi(chi)
        got = h.time_gradient()
    otr.assert_time_gradient_agrees(got, want_chi, None, "caller's chi, no target")
    # chi = c_k sigma_k of the built-in functional: the built-in result
    _, c = orf.functional_values(want["tau"], pr.get("weights"), RE)
    with _open(g, pr) as h:
        h.eval(x)
        builtin = h.time_gradient()
        h.forward(x)
        h.backward_chi(np.asarray(c, complex)[:, None, None] * pr["target"])
        through_chi = h.time_gradient()
        h.eval(x)
        again = h.time_gradient()        # ... and the handle remembers which of the two the LAST backward half used
    otr.assert_time_gradient_agrees(builtin, want["dJdt"], want["tau"], "built-in")
    otr.assert_time_gradient_agrees(through_chi, want["dJdt"], want["tau"], "c_k sigma_k through backward_chi")
    assert np.array_equal(again, builtin)


# ---- 7. the state machine -----------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason_and_leave_the_handle_usable(g):
    from grape_jl_amd import synth
    pr = synth.make_open_problem(5, 2, 3, 2, 2, seed=905)
    pr["functional"] = SM
    x = pr["pulsevals"]
    out = np.zeros(3)
    p = out.ctypes.data
    with _open(g, pr) as h:
        lib, hd = h._lib, h._h

        def refused(needle, call=lambda: lib.grape_open_time_gradient(hd, p), handle=hd):
            assert call() == -1, needle
            msg = lib.grape_last_error(handle)
            assert b"grape_open_time_gradient" in msg and needle in msg, (needle, msg)

        refused(b"no evaluation")
        first = h.eval(x)
        tg = h.time_gradient()

        def same_bits():
            J, G, tau = h.eval(x)
            assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(tau, first[2])
            assert np.array_equal(h.time_gradient(), tg)

        refused(b"h == NULL", lambda: lib.grape_open_time_gradient(None, p), None)
        same_bits()
        refused(b"dJdt == NULL", lambda: lib.grape_open_time_gradient(hd, None))
        same_bits()
        h.eval(x, gradient=False)
        refused(b"had no gradient")
        same_bits()
        h.forward(x)
        refused(b"between grape_forward and the backward half")
        h.backward(complex(*h.sums()[:2]))
        assert np.array_equal(h.time_gradient(), tg)      # forward + backward is eval
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
            h.time_gradient()
        assert err.value.code == -1 and "grape_set_tlist" in str(err.value)
        same_bits()
        h.check()
    cl = synth.make_problem(5, 2, 3, 2, seed=77)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"]) as hc:
        Jc, Gc, _ = hc.eval(cl["pulsevals"])
        assert hc._lib.grape_open_time_gradient(hc._h, p) == -1
        msg = hc._lib.grape_last_error(hc._h)
        assert b"grape_get_time_gradient" in msg and b"not an open-system handle" in msg
        tgc = hc.time_gradient()
        J2, G2, _ = hc.eval(cl["pulsevals"])
        assert J2 == Jc and np.array_equal(G2, Gc) and np.array_equal(hc.time_gradient(), tgc)


# ---- 8. non-interference and repeatability -------------------------------------------------------------------------------------
def test_the_call_disturbs_nothing_and_repeats_bitwise(g):
    name = "d33_J7_L5_re"
    pr, want = otr.reference_of(name, CASES)
    x = pr["pulsevals"]
    rng = np.random.default_rng(33)
    t2 = _tlist(rng.uniform(0.4, 1.6, 3))
    with _open(g, pr) as h:
        J, G, tau = h.eval(x)
        before = dict(tg=h.tau_grads(), work=h.work(), timings=h.timings(), store=h.storage(0))
        a = h.time_gradient()
        b = h.time_gradient()
        after = dict(tg=h.tau_grads(), work=h.work(), timings=h.timings(), store=h.storage(0))
        assert np.array_equal(a, b)
        assert np.array_equal(before["tg"], after["tg"]) and np.array_equal(before["store"], after["store"])
        assert before["work"] == after["work"] and before["timings"] == after["timings"]
        assert before["timings"]["forward"] > 0.0 and before["work"]["series_terms"] > 0
        J1, G1, tau1 = h.eval(x)
        assert J1 == J and np.array_equal(G1, G) and np.array_equal(tau1, tau)
        assert np.array_equal(h.tau_grads(), before["tg"])
        assert np.array_equal(h.time_gradient(), a)
        h.set_tlist(t2)
        Jm, Gm, _ = h.eval(x)
        moved = h.time_gradient()
    with _open(g, dict(pr, tlist=t2)) as h:
        Jf, Gf, _ = h.eval(x)
        fresh = h.time_gradient()
    otr.assert_time_gradient_agrees(a, want["dJdt"], want["tau"], name)
    assert Jm == Jf and np.array_equal(Gm, Gf) and np.array_equal(moved, fresh)
    assert Jm != J and not np.array_equal(moved, a)
