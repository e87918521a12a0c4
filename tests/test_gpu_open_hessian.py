"""grape_open_hessian: the exact Hessian of J as a matrix on open-system handles (csrc/grape_lindblad_hessian.hip.h) -- needs
an MI355X.

Against the adjoint-form reference of tests/open_hessian_reference.py (proved against the forward-over-forward reference by
tests/test_open_hessian_reference.py) on every NP = 16 / 32 / 48 / 64 instantiation, and against grape_open_hvp with the
identity on the same handle; bitwise symmetry; sub-steps; pass size and fan block size; repetition; non-interference; every
refusal; the optimiser the call is for.

The comparison with the reference is open_hessian_reference.assert_open_hessian_agrees:
    ||dH||_inf <= 1e-10 max(||H||_inf, 1e-3)                    (the project's bar for H v)
after asserting ON THE REFERENCE ALONE min_k |tau_k| >= 0.1, ||G||_inf >= 1e-3, ||H||_inf >= 1e-3: the bound is relative, never its floor.
The shapes are the smallest that reach every instantiation; on each the fan entries with n - m >= 2 are at least 1e-3.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
import open_hessian_reference as ohs  # noqa: E402
import open_hvp_reference as ohr  # noqa: E402
from open_hessian_reference import RE, SM, SS  # noqa: E402

pytestmark = pytest.mark.gpu

THETA = 3.0   # sub-step threshold of the kernels


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


GRID = dict(weights=True, shape=True, nonuniform=True)
CASES = {
    "d3": dict(d=3, J=2, L=2, K=2, N_T=6, functional=SM, **GRID),                                      # NP 16, padded rows
    "d16": dict(d=16, J=1, L=3, K=2, N_T=6, functional=SS, nonuniform=True),                           # NP 16 full tile, L = 3
    "d17": dict(d=17, J=2, L=4, K=3, N_T=5, functional=SM, **GRID),                                    # NP 32, ten pairs, K = 3
    "d33": dict(d=33, J=3, L=2, K=2, N_T=5, functional=RE, hermitian=False, non_hermitian_states=0.3, nonuniform=True),   # NP 48, general drift
    "d48": dict(d=48, J=0, L=2, K=2, N_T=5, functional=SS, hc_per_traj=True, nonuniform=True),         # NP 48 full, no dissipator
    "d49": dict(d=49, J=1, L=2, K=2, N_T=5, functional=SM, cops_per_traj=True, **GRID),                # NP 64 padded
    "d64": dict(d=64, J=2, L=2, K=2, N_T=5, functional=SM, **GRID),                                    # NP 64 full
    "d64J8": dict(d=64, J=8, L=2, K=2, N_T=4, functional=SM, factor=-0.8, **GRID),                     # J = 8 at NP 64
}


def _open(g, pr, functional=None, **kw):
    return g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr.get("target"), pr.get("weights"),
                          functional=pr["functional"] if functional is None else functional, shape=pr.get("shape"), **kw)


def _tlist(dts):
    return np.concatenate([[0.0], np.cumsum(dts)])


def _far_entries(H, L, N_T):
    """the entries of H (p = l N_T + n) whose intervals lie at least two apart: what only a carried column can give"""
    n = np.arange(L * N_T) % N_T
    return H[np.abs(n[:, None] - n[None, :]) >= 2]


# ---- 1. against the reference and against grape_open_hvp ------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference_and_the_unit_direction_route(g, name):
    pr, want = ohs.reference_of(name, CASES)
    K, L, N_T = pr["H0"].shape[0], np.asarray(pr["Hc"]).shape[-3], len(pr["tlist"]) - 1
    P = L * N_T
    assert np.abs(_far_entries(want["H"], L, N_T)).max() >= 1e-3
    with _open(g, pr) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        H = h.open_hessian()
        info = h.open_hessian_info()
        unit = h.open_hvp(np.eye(P))
    assert abs(J - want["J"]) <= oh.TOL_J and np.abs(tau - want["tau"]).max() <= oh.TOL_TAU
    assert np.abs(G - want["G"]).max() <= oh.tol_G(want["G"])
    ohs.assert_open_hessian_agrees(H, want, name)
    ohr.assert_open_hvp_agrees(H, dict(tau=want["tau"], G=want["G"], Hv=unit), name + " against open_hvp(identity)")
    assert np.array_equal(H, H.T)
    pairs = L * (L + 1) // 2
    assert info["steps_forward_seeds"] >= K * L * N_T and info["steps_backward_seeds"] >= K * (1 + pairs) * N_T    # (theta chain + pairs)
    assert info["steps_fan"] >= K * L * (N_T - 1) * (N_T - 2) // 2            # column (m, l') is carried through N_T - 2 - m intervals
    assert info["series_terms"] == info["terms_forward_seeds"] + info["terms_backward_seeds"] + info["terms_fan"] > 0
    assert info["series_steps"] == info["steps_forward_seeds"] + info["steps_backward_seeds"] + info["steps_fan"]
    assert info["traj_per_pass"] == K and info["bytes"] > 0 and info["ms"] > 0.0 and info["fan_columns"] == 1


def _kernel_beta(pr, k, n):
    """beta_n of the kernels' sub-step rule, up to their norm estimate: 1.1 x a power-iteration value that
    lies a few per cent below the 2-norm at most"""
    n2 = lambda A: np.linalg.norm(A, 2)   # noqa: E731
    L, N_T = pr["Hc"].shape[0], len(pr["tlist"]) - 1
    e = np.abs(pr["pulsevals"].reshape(L, N_T)[:, n])
    return 1.1 * (2.0 * (n2(pr["H0"][k]) + sum(e[l] * n2(pr["Hc"][l]) for l in range(L)))) + 1.21 * sum(n2(A) ** 2 for A in pr["cops"])


def test_d48_one_interval_of_three_substeps(g):
    """d = 48, J = 8, L = 1, K = 1, J_T_ss: interval 1 has beta dt / theta just above 2 (2.25, with the 5 % the norm estimate may lie
    lower: three sub-steps), the outer ones one sub-step each; the counts are asserted from the info call.  The one carried
    column (born at t_1) crosses exactly the cut interval"""
    from grape_jl_amd import synth
    d, L, K, N_T = 48, 1, 1, 3
    pr = synth.make_open_problem(d, L, N_T, K, 8, seed=4808)
    beta = _kernel_beta(pr, 0, 1)
    dt1, dt0 = 2.25 * THETA / beta, 0.3 * THETA / beta
    assert 2 < 0.95 * beta * dt1 / THETA and beta * dt1 / THETA < 3
    pr["tlist"] = _tlist([dt0, dt1, dt0])
    pr["functional"] = SS
    oh.order_one_states(pr, 4808, factor=-0.8)
    x = pr["pulsevals"]
    want = ohs.evaluate(pr, x, SS)
    with _open(g, pr) as h:
        h.eval(x)
        H = h.open_hessian()
        info = h.open_hessian_info()
    ohs.assert_open_hessian_agrees(H, want, "d48, three sub-steps")
    assert np.array_equal(H, H.T)
    # (the backward count holds the bare target chain and the one pair: twice the five (sub-)steps)
    assert info["steps_forward_seeds"] == 1 + 3 + 1 and info["steps_backward_seeds"] == 2 * (1 + 3 + 1) and info["steps_fan"] == 3


def seed_rows(K, L, N_T):
    """workgroups along the intervals of the forward seeds | of the backward seeds (open_hess_seed_rows, open_hess_back_rows of
    csrc/grape_hip.hip, restated: the long case below is chosen by them, the two move together)"""
    pairs = L * (L + 1) // 2
    return max(1, min(N_T, -(-1024 // (K * L)))), max(1, min(N_T, -(-512 // (K * pairs))))


LONG = dict(d=3, J=1, L=2, K=2, N_T=300, functional=SS, dt=0.5, weights=True, shape=True)


def test_a_long_grid_where_the_seed_workgroups_take_several_intervals(g):
    """The table above has K L N_T <= 1024 and K pairs N_T <= 512: every seed workgroup takes one interval.  N_T = 300 at K = 2,
    L = 2: 256 forward rows (a second trip for 44 of them) and 86 backward rows (three or four trips each), 600 carried columns,
    the first across 298 intervals"""
    K, L, N_T = LONG["K"], LONG["L"], LONG["N_T"]
    rows_f, rows_b = seed_rows(K, L, N_T)
    assert rows_f == 256 < N_T and rows_b == 86 and 3 * rows_b < N_T
    if "long" not in ohs._CACHE:
        import open_time_reference as otr
        pr = otr.build_case(LONG)
        ohs._CACHE["long"] = (pr, ohs.evaluate(pr, pr["pulsevals"], pr["functional"]))
    pr, want = ohs._CACHE["long"]
    P = L * N_T
    assert np.abs(_far_entries(want["H"], L, N_T)).max() >= 1e-3
    with _open(g, pr) as h:
        h.eval(pr["pulsevals"])
        H = h.open_hessian()
        info = h.open_hessian_info()
        unit = h.open_hvp(np.eye(P))
    ohs.assert_open_hessian_agrees(H, want, "N_T 300")
    ohr.assert_open_hvp_agrees(H, dict(tau=want["tau"], G=want["G"], Hv=unit), "N_T 300 against open_hvp(identity)")
    assert np.array_equal(H, H.T)
    assert info["steps_forward_seeds"] >= K * L * N_T and info["steps_backward_seeds"] >= K * 4 * N_T and info["fan_columns"] == 1


# ---- 2. passes, blocks, repetition, routes ----------------------------------------------------------------------------------------
def test_pass_size_and_fan_blocks_never_change_a_bit(g, monkeypatch):
    """K = 3 in one pass against passes of one and of two trajectories (GRAPE_OPEN_HESS_TRAJ, read at create), and one column
    per fan workgroup against three (P = 20: staggered births inside a block, a last block of two) and sixteen
    (GRAPE_OPEN_HESS_COLS): bit for bit.  Two calls give the same bits."""
    pr, want = ohs.reference_of("d17", CASES)
    x = pr["pulsevals"]
    with _open(g, pr) as h:
        h.eval(x)
        one_pass = h.open_hessian()
        info = h.open_hessian_info()
        again = h.open_hessian()
        assert h.open_hessian_info()["bytes"] == info["bytes"]
    assert info["traj_per_pass"] == 3 and info["fan_columns"] == 1
    assert np.array_equal(one_pass, again)
    for traj in (1, 2):
        monkeypatch.setenv("GRAPE_OPEN_HESS_TRAJ", str(traj))
        with _open(g, pr) as h:
            h.eval(x)
            passes = h.open_hessian()
            pinfo = h.open_hessian_info()
        monkeypatch.delenv("GRAPE_OPEN_HESS_TRAJ")
        assert pinfo["traj_per_pass"] == traj and 0 < pinfo["bytes"] < info["bytes"]
        assert pinfo["series_terms"] == info["series_terms"] and pinfo["series_steps"] == info["series_steps"]
        assert np.array_equal(one_pass, passes)
    for cols in (3, 16):
        monkeypatch.setenv("GRAPE_OPEN_HESS_COLS", str(cols))
        with _open(g, pr) as h:
            h.eval(x)
            blocks = h.open_hessian()
            binfo = h.open_hessian_info()
        monkeypatch.delenv("GRAPE_OPEN_HESS_COLS")
        assert binfo["fan_columns"] == cols and binfo["series_terms"] == info["series_terms"]
        assert np.array_equal(one_pass, blocks)
    ohs.assert_open_hessian_agrees(one_pass, want, "d17")


def test_every_route_to_a_forward_state_gives_the_same_bits(g):
    pr, want = ohs.reference_of("d16", CASES)
    x = pr["pulsevals"]
    with _open(g, pr) as h:
        h.eval(x)
        full = h.open_hessian()
        h.eval(x, gradient=False)
        no_gradient = h.open_hessian()
        h.forward(x)
        forward_only = h.open_hessian()
    assert np.array_equal(full, no_gradient) and np.array_equal(full, forward_only)


# ---- 3. non-interference ----------------------------------------------------------------------------------------------------------
def test_the_call_disturbs_nothing(g):
    pr, want = ohs.reference_of("d33", CASES)
    x = pr["pulsevals"]
    d = pr["H0"].shape[1]
    V = ohr.directions(33, 2, x.size)
    ops = np.stack([np.diag(np.arange(d, dtype=float)).astype(complex), pr["target"][0]])
    with _open(g, pr) as h:
        J, G, tau = h.eval(x)

        def state():
            return dict(tg=h.tau_grads(), work=h.work(), timings=h.timings(), store=h.storage(0), dJdt=h.time_gradient(), ex=h.expect(ops))

        hv = h.open_hvp(V)
        hv_info = h.open_hvp_info()
        dtau, dsums = h.open_hvp_forward(V)
        halves = h.open_hvp_backward(complex(*h.sums()[:2]), dsums)
        before = state()
        h.open_hvp_forward(V)                       # a pending backward half ...
        H = h.open_hessian()
        pending = h.open_hvp_backward(complex(*h.sums()[:2]), dsums)     # ... still answers
        after = state()
        assert np.array_equal(pending, halves)
        for key in ("tg", "store", "dJdt", "ex"):
            assert np.array_equal(before[key], after[key]), key
        assert before["work"] == after["work"] and before["timings"] == after["timings"]
        assert np.array_equal(h.open_hvp(V), hv) and h.open_hvp_info()["bytes"] == hv_info["bytes"]
        J1, G1, tau1 = h.eval(x)
        assert J1 == J and np.array_equal(G1, G) and np.array_equal(tau1, tau)
        assert np.array_equal(h.tau_grads(), before["tg"]) and np.array_equal(h.time_gradient(), before["dJdt"])
        assert np.array_equal(h.expect(ops), before["ex"])
        assert np.array_equal(h.open_hessian(), H)
    ohs.assert_open_hessian_agrees(H, want, "d33")


# ---- 4. refusals and errors ---------------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason_and_leave_the_handle_usable(g):
    import open_time_reference as otr
    from grape_jl_amd import synth
    pr, want = ohs.reference_of("d3", CASES)
    x = pr["pulsevals"]
    P = x.size
    out = np.zeros((P, P))
    po = out.ctypes.data
    with _open(g, pr) as h:
        lib, hd = h._lib, h._h

        def refused(needle, call=lambda: lib.grape_open_hessian(hd, po), handle=hd):
            assert call() == -1, needle
            msg = lib.grape_last_error(handle)
            assert msg.startswith(b"grape_open_hessian:") and needle in msg, (needle, msg)

        refused(b"no evaluation")
        first = h.eval(x)
        tg = h.tau_grads()
        H = h.open_hessian()

        def same_bits():
            J, G, tau = h.eval(x)
            assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(tau, first[2])
            assert np.array_equal(h.tau_grads(), tg) and np.array_equal(h.open_hessian(), H)

        refused(b"h == NULL", lambda: lib.grape_open_hessian(None, po), None)
        same_bits()
        refused(b"H must not be NULL", lambda: lib.grape_open_hessian(hd, None))
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
        # a running cost: set (the stored states are stale), evaluated (its second-order terms are not carried), removed
        h.set_running_cost(pr["target"][0], 0.1)
        refused(b"grape_open_set_running_cost")
        h.eval(x)
        refused(b"running cost")
        h.set_running_cost(None, 0.0)
        refused(b"grape_open_set_running_cost came after")
        same_bits()
        with pytest.raises(g.GrapeHipError) as err:      # the Python method raises what the library says
            h.set_tlist(pr["tlist"])
            h.open_hessian()
        assert err.value.code == -1 and "grape_set_tlist" in str(err.value)
        same_bits()
        h.check()
    # a split-phase shard, and a handle without targets
    with _open(g, dict(pr, H0=pr["H0"][:1], rho0=pr["rho0"][:1], target=pr["target"][:1], weights=pr["weights"][:1]), K_total=2) as hs:
        hs.forward(x)
        assert hs._lib.grape_open_hessian(hs._h, po) == -1
        assert b"K < K_total" in hs._lib.grape_last_error(hs._h)
        hs.backward(complex(*hs.sums()[:2]))
    with _open(g, dict(pr, target=None)) as hn:
        hn.forward(x)
        assert hn._lib.grape_open_hessian(hn._h, po) == -1
        assert b"no target states" in hn._lib.grape_last_error(hn._h)
        hn.forward(x)
    # L = 5 (the message names the route), and L N_T = 8194
    p5 = otr.build_case(dict(d=3, J=1, L=5, K=1, functional=RE))
    big = np.zeros((15, 15))
    with _open(g, p5) as h5:
        J5, G5, _ = h5.eval(p5["pulsevals"])
        assert h5._lib.grape_open_hessian(h5._h, big.ctypes.data) == -1
        msg = h5._lib.grape_last_error(h5._h)
        assert msg.startswith(b"grape_open_hessian:") and b"L > 4" in msg and b"grape_open_hvp with unit directions" in msg
        J6, G6, _ = h5.eval(p5["pulsevals"])
        assert J6 == J5 and np.array_equal(G6, G5) and h5.open_hvp(np.eye(15)).shape == (15, 15)
    pl = otr.build_case(dict(d=3, J=1, L=2, K=1, N_T=4097, functional=RE, dt=0.01))
    with _open(g, pl) as hl:
        Jl, Gl, _ = hl.eval(pl["pulsevals"])
        assert hl._lib.grape_open_hessian(hl._h, po) == -1            # (refused before H is touched)
        msg = hl._lib.grape_last_error(hl._h)
        assert msg.startswith(b"grape_open_hessian:") and b"L * N_T > 8192" in msg
        Jm, Gm, _ = hl.eval(pl["pulsevals"])
        assert Jm == Jl and np.array_equal(Gm, Gl)
    # a closed handle: the message names grape_hessian; grape_hessian on an open handle still names grape_open_hvp
    cl = synth.make_problem(5, 2, 3, 2, seed=77)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"]) as hc:
        Jc, Gc, _ = hc.eval(cl["pulsevals"])
        Hc = hc.hessian()
        assert hc._lib.grape_open_hessian(hc._h, po) == -1
        msg = hc._lib.grape_last_error(hc._h)
        assert msg.startswith(b"grape_open_hessian:") and b"grape_hessian" in msg and b"not an open-system handle" in msg
        assert hc._lib.grape_get_open_hessian_info(hc._h, po, 12) == -1
        J2, G2, _ = hc.eval(cl["pulsevals"])
        assert J2 == Jc and np.array_equal(G2, Gc) and np.array_equal(hc.hessian(), Hc)
    with _open(g, pr) as h:
        h.eval(x)
        assert h._lib.grape_hessian(h._h, po) == -1
        msg = h._lib.grape_last_error(h._h)
        assert msg.startswith(b"grape_hessian:") and b"open-system" in msg and b"grape_open_hvp with unit directions" in msg
        assert np.array_equal(h.open_hessian(), H)


def test_a_series_that_cannot_converge_is_grape_err_taylor(g):
    """The over-long interval of tests/test_gpu_open_reference.py stops the EVALUATION with GRAPE_ERR_TAYLOR, so this call refuses
    (no valid forward state: the last forward sweep failed); back on the sane grid the handle gives its first matrix bit for bit.
    The call's own GRAPE_ERR_TAYLOR needs a valid forward state and a series that cannot converge.  grape_open_hvp reaches
    that with a direction that is not finite; this call takes no vector from the caller -- pulses, grid and operators are those
    the forward sweep has just summed to convergence -- so no input of the public interface reaches it."""
    pr, want = ohs.reference_of("d3", CASES)
    x = pr["pulsevals"]
    bad = pr["tlist"].copy()
    bad[2:] += 1e6 - 1.0
    with _open(g, pr) as h:
        first = h.eval(x)
        H = h.open_hessian()
        h.set_tlist(bad)
        with pytest.raises(g.GrapeHipError) as err:
            h.eval(x)
        assert err.value.code == -5
        with pytest.raises(g.GrapeHipError) as err:
            h.open_hessian()
        assert err.value.code == -1 and "failed" in str(err.value)
        h.set_tlist(pr["tlist"])                       # the sane grid again
        J, G, tau = h.eval(x)
        assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(tau, first[2])
        assert np.array_equal(h.open_hessian(), H)
        h.check()


# ---- 5. the optimiser the call is for -----------------------------------------------------------------------------------------------
def test_trust_exact_drives_a_dissipative_state_transfer(g):
    """The d = 3 ladder with amplitude damping of tests/test_gpu_open_hvp.py (|0><0| -> |1><1| under J_T_re): scipy's trust-exact
    with hess = GrapeHipOpen.open_hessian reaches the final J of trust-ncg with hessp = open_hvp from the same start.  Both
    stop at ||G|| <= 1e-9; at a minimum with curvature lambda the distance in J is ||G||^2 / (2 lambda) -- 1e-8 leaves room
    for lambda down to 5e-11"""
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

        def ensure(x):
            if not np.array_equal(x, at[0]):      # (after a rejected trial step the handle holds the trial point's states)
                h.eval(x, gradient=False)
                at[0] = x.copy()

        def hessp(x, p):
            ensure(x)
            return h.open_hvp(p)

        def hess(x):
            ensure(x)
            return h.open_hessian()

        J0 = fg(x0)[0]
        nc = scipy.optimize.minimize(fg, x0, jac=True, hessp=hessp, method="trust-ncg", options=dict(gtol=1e-9, maxiter=200))
        te = scipy.optimize.minimize(fg, x0, jac=True, hess=hess, method="trust-exact", options=dict(gtol=1e-9, maxiter=200))
    print(dict(J0=J0, trust_ncg=nc.fun, nit_ncg=nc.nit, trust_exact=te.fun, nit_exact=te.nit, nhev=te.nhev))
    assert nc.fun < 0.5 * J0 and te.fun > 0.0           # a real descent, to a decoherence-limited optimum (J > 0)
    assert te.fun <= nc.fun + 1e-8
