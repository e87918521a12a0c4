"""grape_hessian on the GPU: the exact Hessian of J as a matrix (include/grape_hip.h, csrc/grape_hessian.hip.h).

Bar: the project's gradient tolerance applied to the entries of H against tests/hessian_reference.py (proved in
tests/test_hessian_reference.py),
    ||dH||_inf <= 1e-10 * max(||H||_inf, 1e-3)   over all entries,
and every case asserts on the reference alone min|tau_k| >= 0.1, ||G||_inf >= 1e-3, ||H||_inf >= 1e-3, so that the bound is
relative and never its floor.  The shapes are the smallest at which each mechanism can go wrong: the table of CASES for
the kernels' arithmetic (paddings, column blocks that straddle intervals, a full backward tile, cut intervals), where every
forward-seed workgroup takes one interval, and the table of LONG_CASES for the launch plan beyond that regime:
  * the stride of the forward seeds: hess_seed_rows (csrc/grape_hip.hip, restated here as ``seed_rows``) deals
    min(N_T, ceil(1024 / K)) workgroups per trajectory, so with K N_T > 1024 a workgroup takes n = g, g + rows, ... -- a second
    trip for some workgroups only (N_T 300, K 4), for every one (N_T 2048, K 1), and all intervals in one workgroup (K 1030);
  * the block count: 38 and 128 column blocks of the fan instead of at most three, columns carried across up to 2047
    intervals, and 1407 and 16384 workgroups of the accumulate and finish kernels instead of at most five;
  * the NULL operands: handles created without weights and without shape (``plain``), under sm and ss.
"Bit for bit" is ``np.array_equal``.
"""
import numpy as np
import pytest

import grape_jl_amd as g
import hessian_reference as hs
import hvp_reference as hr
from grape_jl_amd import synth

pytestmark = pytest.mark.gpu


def make_case(N, L, N_T, K, seed, herm=True, per_traj=False, skew=0, dt=1.0, amp=3.0, uniform=False, plain=False):
    """weights, shape and a non-uniform grid throughout (``uniform``: every interval is dt long; ``plain``: neither weights
    nor shape, the handle gets NULL for both)"""
    pr = synth.make_problem(N, L, N_T, K, seed=seed, hermitian=herm, dt=dt)
    pr["pulsevals"] = amp * pr["pulsevals"]
    if per_traj:
        pr["Hc"] = np.stack([np.stack([synth.gue(synth.subseed(seed, 500 + 10 * k + l), N) for l in range(L)]) for k in range(K)])
    if not herm:   # general control operators as well
        z = synth.normal(synth.subseed(seed, 8), 2 * N * N)
        pr["Hc"] = pr["Hc"] + 0.1 * (z[0::2] + 1j * z[1::2]).reshape(N, N) / np.sqrt(N)
    if skew:       # badly scaled: S H S^-1 with S = diag(2^e), so that the balancing of the handle is not the identity
        e = (synth.splitmix64(synth.subseed(seed, 11), N) % np.uint64(2 * skew + 1)).astype(np.int64) - skew
        e[0], e[-1] = -skew, skew
        S = 2.0 ** e
        pr["H0"] = S[:, None] * pr["H0"] / S[None, :]
        pr["Hc"] = S[:, None] * pr["Hc"] / S[None, :]
        pr["psi0"] = pr["psi0"] * S[None, :]
        pr["psi0"] /= np.linalg.norm(pr["psi0"], axis=1, keepdims=True)
    u = synth.uniform01(synth.subseed(seed, 8100), N_T + L * N_T + K)
    if not uniform:
        pr["tlist"] = np.concatenate([[0.0], np.cumsum(dt * (0.5 + u[:N_T]))])
    pr["shape"] = 0.5 + 0.5 * u[N_T:N_T + L * N_T].reshape(L, N_T)
    pr["weights"] = 0.5 + u[N_T + L * N_T:]
    if plain:
        pr["shape"] = None
        pr["weights"] = None
    hr.order_one_targets(pr)
    return pr


def handle(pr, functional, **kw):
    return g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=functional,
                      shape=pr["shape"], **kw)


CASES = {
    # two column blocks (20 columns), the second born mid-pulse
    "N3-L1-NT20-K2-sm": dict(N=3, L=1, N_T=20, K=2, f=0),
    # 33 columns: three blocks that straddle intervals (L = 3)
    "N17-L3-NT11-K3-sm": dict(N=17, L=3, N_T=11, K=3, f=0),
    # 1 + 4 + 10 = 15 columns: the backward tile is full
    "N16-L4-NT5-K2-re": dict(N=16, L=4, N_T=5, K=2, f=2, amp=1.5),
    # general generator, rows and columns scaled by 2^+-3
    "N33-L2-NT9-K2-ss-general-skewed": dict(N=33, L=2, N_T=9, K=2, f=1, herm=False, skew=3),
    "N40-L2-NT9-K2-ss-pertraj": dict(N=40, L=2, N_T=9, K=2, f=1, per_traj=True),
    # intervals of length 4: every interval is cut into sub-steps
    "N48-L1-NT18-K1-ss-long-intervals": dict(N=48, L=1, N_T=18, K=1, f=1, dt=4.0, uniform=True),
    "N64-L2-NT9-K1-sm": dict(N=64, L=2, N_T=9, K=1, f=0),
}


def seed_rows(K, N_T):
    """workgroups of the forward seeds per trajectory: hess_seed_rows of csrc/grape_hip.hip restated.  Below N_T, workgroup
    g takes the intervals n = g, g + rows, ..."""
    return max(1, min(N_T, (1024 + K - 1) // K))


# beyond one interval per forward-seed workgroup, three column blocks and five element workgroups; NULL weights and shape
LONG_CASES = {
    # rows = 256 < 300: the workgroups g < 44 take two intervals, the rest one; 38 column blocks; 1407 element workgroups
    "N3-L2-NT300-K4-sm-strided-seeds": dict(N=3, L=2, N_T=300, K=4, f=0),
    # rows = 26 < 30 with many trajectories: the boundary term of ss over 40 of them
    "N5-L1-NT30-K40-ss-strided-seeds": dict(N=5, L=1, N_T=30, K=40, f=1),
    # rows = 1: one workgroup per trajectory loops over all intervals; grid.x = 1030; the boundary term of sm over 1030
    "N2-L1-NT3-K1030-sm-one-seed-row": dict(N=2, L=1, N_T=3, K=1030, f=0),
    # rows = 1024: every workgroup takes exactly two intervals; 128 column blocks; carries across 2047 intervals; 16384
    # element workgroups
    "N2-L1-NT2048-K1-re-two-intervals-per-seed": dict(N=2, L=1, N_T=2048, K=1, f=2, dt=0.25),
    # NULL weights and shape: the coefficient and the boundary term of sm, then ss with a full backward tile
    "N20-L3-NT12-K2-sm-plain": dict(N=20, L=3, N_T=12, K=2, f=0, plain=True, uniform=True),
    "N17-L4-NT6-K2-ss-plain": dict(N=17, L=4, N_T=6, K=2, f=1, plain=True, uniform=True, amp=1.5),
}
STRIDED = list(LONG_CASES)[:4]
_cache = {}


def case(name):
    """(problem, functional, reference): computed once and shared, never modified"""
    if name not in _cache:
        c = dict(CASES[name] if name in CASES else LONG_CASES[name])
        f = c.pop("f")
        pr = make_case(seed=2000 + sum(map(ord, name)), **c)
        _cache[name] = (pr, f, hs.evaluate(pr, pr["pulsevals"], f))
    return _cache[name]


def uncut_steps(L, N_T, K):
    """(sub-)steps of one call when no interval is cut: K N_T forward seeds, K N_T backward seeds, and every column block of
    the fan from the interval after the birth of its first column to the last but one"""
    fan = sum(max(0, N_T - 1 - ((16 * b) // L + 1)) for b in range((L * N_T + 15) // 16))
    return K * (2 * N_T + fan)


def probe_columns(L, N_T, K):
    """the columns of H (p = l N_T + n) where the launch plan changes, from the shape alone.  The fan and the seeds count
    interval-major, q = n L + l: the first and the last column, both sides of the first column-block boundary (q = 15, 16),
    the first and last control on both sides of the seed stride (n = rows - 1, rows), one column of the interior (q = P / 3).
    At most nine."""
    P, rows = L * N_T, seed_rows(K, N_T)
    qs = [0, P - 1, 15, 16] + [n * L + l for n in (rows - 1, rows) for l in (0, L - 1)] + [P // 3]
    qs = list(dict.fromkeys(q for q in qs if 0 <= q < P))
    return np.array([(q % L) * N_T + q // L for q in qs])


@pytest.mark.parametrize("name", list(CASES))
def test_hessian_against_the_reference(name):
    pr, f, want = case(name)
    hs.assert_order_one(want)
    P = pr["L"] * pr["N_T"]
    with handle(pr, f) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        H = h.hessian()
        info = h.hessian_info()
        Hv = h.hvp(np.eye(P))
    assert abs(J - want["J"]) <= 1e-12 and np.abs(G - want["G"]).max() <= hr.tol_hv(want["G"])
    assert H.shape == (P, P)
    hs.assert_hessian_agrees(H, want["H"], name)
    # on the device: column q is grape_hvp of the unit direction e_q (H symmetric: rows and columns alike)
    hs.assert_hessian_agrees(H, Hv, name + " against grape_hvp(identity)")
    assert np.array_equal(H, H.T)
    print(info)
    steps = uncut_steps(pr["L"], pr["N_T"], pr["K"])
    if name == "N48-L1-NT18-K1-ss-long-intervals":
        # beta_n dt_n / theta: the norm estimate of the generator is ~ 1 plus the control, every interval is 4 long and
        # theta = 3, so every interval is cut at least once
        assert info["series_steps"] >= 2 * steps, (info, steps)
    else:
        assert info["series_steps"] >= steps, (info, steps)
    assert info["series_terms"] == info["terms_forward_seeds"] + info["terms_backward_seeds"] + info["terms_fan"]
    assert min(info["terms_forward_seeds"], info["terms_backward_seeds"], info["terms_fan"]) > 0
    assert info["traj_per_pass"] == pr["K"] and info["bytes"] > 0 and info["ms"] > 0


@pytest.mark.parametrize("name", list(LONG_CASES))
def test_hessian_beyond_one_interval_per_seed_workgroup(name):
    """LONG_CASES against the reference (proved at these lengths in tests/test_hessian_reference.py), and against grape_hvp
    on the columns where the launch plan changes.  Worst dH / tol on the device: docs/LAB_NOTEBOOK.md"""
    pr, f, want = case(name)
    L, N_T, K = pr["L"], pr["N_T"], pr["K"]
    P, rows = L * N_T, seed_rows(K, N_T)
    if name in STRIDED:
        assert rows < N_T, (rows, N_T)           # from the inputs alone: the case reaches the strided loop
    else:
        assert pr["weights"] is None and pr["shape"] is None
    hs.assert_order_one(want)
    cols = probe_columns(L, N_T, K)
    assert 1 <= len(cols) <= 16 and len(set(cols)) == len(cols)
    E = np.zeros((len(cols), P))
    E[np.arange(len(cols)), cols] = 1.0
    with handle(pr, f) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        H = h.hessian()
        info = h.hessian_info()
        Hv = h.hvp(E)
    print(name, dict(dJ=abs(J - want["J"]), dG=float(np.abs(G - want["G"]).max()), tol_G=hr.tol_hv(want["G"])))
    assert abs(J - want["J"]) <= 1e-12 and np.abs(G - want["G"]).max() <= hr.tol_hv(want["G"])
    assert H.shape == (P, P)
    dev = hs.assert_hessian_agrees(H, want["H"], name)
    print(name, "worst dH / tol = %.3g" % (dev / hs.tol_hessian(want["H"])))
    assert np.array_equal(H, H.T)
    # on the device: column p is grape_hvp of the unit direction e_p
    hs.assert_hessian_agrees(H[cols], Hv, name + " against grape_hvp(unit directions %s)" % cols.tolist())
    print(info)
    steps = uncut_steps(L, N_T, K)
    assert info["series_steps"] >= steps, (info, steps)
    assert info["series_terms"] == info["terms_forward_seeds"] + info["terms_backward_seeds"] + info["terms_fan"]
    assert min(info["terms_forward_seeds"], info["terms_backward_seeds"], info["terms_fan"]) > 0
    assert info["traj_per_pass"] == K


def test_passes_on_a_strided_shape_give_the_same_bits(monkeypatch):
    """K = 4 with strided seeds: passes of 3 + 1 trajectories and four passes of one against the default single pass"""
    pr, f, _ = case("N3-L2-NT300-K4-sm-strided-seeds")
    assert seed_rows(pr["K"], pr["N_T"]) < pr["N_T"]
    got = {}
    for traj, reported in ((None, 4), ("3", 3), ("1", 1)):
        if traj:
            monkeypatch.setenv("GRAPE_HESS_TRAJ", traj)
        with handle(pr, f) as h:
            h.eval(pr["pulsevals"])
            got[traj] = h.hessian()
            assert h.hessian_info()["traj_per_pass"] == reported
            assert np.array_equal(h.hessian(), got[traj])
    assert np.array_equal(got["3"], got[None]) and np.array_equal(got["1"], got[None])


@pytest.mark.parametrize("name", ["N3-L1-NT20-K2-sm", "N64-L2-NT9-K1-sm"])
def test_hessian_from_the_stored_states_of_the_default_route(monkeypatch, name):
    """without the session's GRAPE_DERIV3=1 pin (tests/test_gpu_default_routes.py) a small problem stores the forward states of
    the scan sweeps and the workgroup-per-batch derivative kernels; the Hessian is taken after the captured graph has replayed"""
    pr, f, want = case(name)
    monkeypatch.setenv("GRAPE_DERIV3", "1")
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        pinned, pinned_kernel = h.hessian(), int(h.work()["asm_deriv_kernel"])
    monkeypatch.delenv("GRAPE_DERIV3")
    with handle(pr, f) as h:
        for _ in range(4):            # (beyond the second evaluation the captured graph replays)
            J, G, tau = h.eval(pr["pulsevals"])
        H, kernel = h.hessian(), int(h.work()["asm_deriv_kernel"])
    if pr["N"] >= 49:                 # (grape_get_work names the derivative kernel from N = 49 on: the two handles took two routes)
        assert (pinned_kernel, kernel) == (1, 0), (pinned_kernel, kernel)
    assert abs(J - want["J"]) <= 1e-12 and np.abs(G - want["G"]).max() <= hr.tol_hv(want["G"])
    hs.assert_hessian_agrees(H, want["H"], name + " default route")
    hs.assert_hessian_agrees(H, pinned, name + " default route against the pinned route")
    print(name, "bit for bit with the pinned route:", np.array_equal(H, pinned))
    assert np.array_equal(H, H.T)


def test_two_calls_and_forced_passes_give_the_same_bits(monkeypatch):
    """two calls bit for bit; GRAPE_HESS_TRAJ=1 (three passes of one trajectory) against the default (one pass of three)"""
    pr, f, _ = case("N17-L3-NT11-K3-sm")
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        H0 = h.hessian()
        assert h.hessian_info()["traj_per_pass"] == 3
        assert np.array_equal(h.hessian(), H0)
    monkeypatch.setenv("GRAPE_HESS_TRAJ", "1")
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        H1 = h.hessian()
        assert h.hessian_info()["traj_per_pass"] == 1
    monkeypatch.setenv("GRAPE_HESS_TRAJ", "2")
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        H2 = h.hessian()
        assert h.hessian_info()["traj_per_pass"] == 2
    assert np.array_equal(H1, H0) and np.array_equal(H2, H0)


def test_route_independence_at_n64():
    """after grape_eval without G, after grape_forward alone and after the matrix-free propagator: each against the reference"""
    pr, f, want = case("N64-L2-NT9-K1-sm")
    got = {}
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"], gradient=False)
        got["eval-no-G"] = h.hessian()
        h.forward(pr["pulsevals"])
        got["forward-alone"] = h.hessian()
    with handle(pr, f, prop_method=g.PROP_SERIES) as h:
        h.eval(pr["pulsevals"])
        got["series"] = h.hessian()
    for tag, H in got.items():
        hs.assert_hessian_agrees(H, want["H"], tag)


def test_no_side_effect_on_the_evaluation_and_the_other_calls():
    pr, f, _ = case("N16-L4-NT5-K2-re")
    V = hr.directions(5, 2, pr["L"] * pr["N_T"])
    for kw in (dict(), dict(prop_method=g.PROP_SERIES)):
        with handle(pr, f, **kw) as h:
            for _ in range(4):        # (beyond the second evaluation the captured graph replays)
                J0, G0, tau0 = h.eval(pr["pulsevals"])
            dJdt0, Hv0 = h.time_gradient(), h.hvp(V)
            ex0 = h.expect(pr["Hc"])
            H0 = h.hessian()
            assert np.array_equal(h.time_gradient(), dJdt0)
            assert np.array_equal(h.hvp(V), Hv0)
            assert np.array_equal(h.expect(pr["Hc"]), ex0)
            for _ in range(3):
                J1, G1, tau1 = h.eval(pr["pulsevals"])
                assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(tau1, tau0)
                assert np.array_equal(h.hessian(), H0)


def test_a_pending_hvp_backward_still_answers():
    pr, f, _ = case("N17-L3-NT11-K3-sm")
    V = hr.directions(6, 2, pr["L"] * pr["N_T"])
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        whole = h.hvp(V)
        f_total = complex(*h.sums()[:2])
        _, dsums = h.hvp_forward(V)
        h.hessian()
        assert np.array_equal(h.hvp_backward(f_total, dsums), whole)


def _refused(h, what):
    with pytest.raises(g.GrapeHipError) as ei:
        h.hessian()
    assert ei.value.code == -1, ei.value
    assert "grape_hessian:" in str(ei.value) and what in str(ei.value), str(ei.value)


def test_refusals_leave_the_handle_usable():
    pr, f, _ = case("N16-L4-NT5-K2-re")
    x, N_T = pr["pulsevals"], pr["N_T"]
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with handle(pr, f) as h:
        _refused(h, "no valid forward state")                        # nothing evaluated yet
        J0, G0, tau0 = h.eval(x)
        H0 = h.hessian()
        assert h._lib.grape_hessian(h._h, None) == -1                # H == NULL
        assert b"grape_hessian:" in h._lib.grape_last_error(h._h) and b"NULL" in h._lib.grape_last_error(h._h)
        h.eval_batch(np.stack([x, 0.9 * x]))
        _refused(h, "grape_eval_batch")
        J1, G1, tau1 = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(tau1, tau0)
        assert np.array_equal(h.hessian(), H0)
        h.set_tlist(pr["tlist"] * 1.25)
        _refused(h, "grape_set_tlist")
        h.set_tlist(pr["tlist"])
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
        assert np.array_equal(h.hessian(), H0)
        # a last backward half with the caller's xi
        h.forward(x)
        h.backward_xi(np.zeros((pr["K"], N_T + 1, pr["N"]), complex), 0.0)
        _refused(h, "caller's xi")
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
        assert np.array_equal(h.hessian(), H0)
    # the built-in running cost
    D = np.diag(np.arange(16.0)).astype(complex)
    with g.GrapeHip(*args, functional=f, D=D, lambda_b=0.1) as h:
        J0, G0, _ = h.eval(x)
        _refused(h, "running cost")
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
    # no targets
    with g.GrapeHip(*args[:4], None, pr["weights"], functional=f) as h:
        h.forward(x)                                                 # (tau is not defined without targets: the final states are)
        psi0 = h.final_states()
        _refused(h, "no target states")
        h.forward(x)
        assert np.array_equal(h.final_states(), psi0)
    # a split-phase shard
    with g.GrapeHip(*args, functional=f, K_total=4) as h:
        tau0 = h.forward(x)
        _refused(h, "shard")
        assert np.array_equal(h.forward(x), tau0)
    # several devices behind one handle (a repeated ordinal)
    with g.GrapeHip(*args, functional=f, devices=[0, 0]) as h:
        J0, G0, _ = h.eval(x)
        _refused(h, "ndev > 1")
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
    # N = 65
    big = synth.make_problem(65, 1, 4, 1, seed=5)
    with g.GrapeHip(big["H0"], big["Hc"], big["tlist"], big["psi0"], big["target"], big["weights"]) as h:
        J0, G0, _ = h.eval(big["pulsevals"])
        _refused(h, "N > 64")
        J1, G1, _ = h.eval(big["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)
    # L = 5: the message names the route
    five = synth.make_problem(4, 5, 4, 1, seed=5)
    with g.GrapeHip(five["H0"], five["Hc"], five["tlist"], five["psi0"], five["target"], five["weights"]) as h:
        J0, G0, _ = h.eval(five["pulsevals"])
        _refused(h, "L > 4")
        _refused(h, "grape_hvp with unit directions")
        J1, G1, _ = h.eval(five["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)
    # L * N_T = 8193
    long = synth.make_problem(2, 1, 8193, 1, seed=5, dt=0.01)
    with g.GrapeHip(long["H0"], long["Hc"], long["tlist"], long["psi0"], long["target"], long["weights"]) as h:
        J0, G0, _ = h.eval(long["pulsevals"])
        _refused(h, "L * N_T > 8192")
        J1, G1, _ = h.eval(long["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)
    # an open-system handle
    op = synth.make_open_problem(4, 1, 4, 1, 1, seed=5)
    with g.GrapeHipOpen(op["H0"], op["Hc"], op["cops"], op["tlist"], op["rho0"], op["target"]) as h:
        J0, G0, _ = h.eval(op["pulsevals"])
        _refused(h, "open-system")
        J1, G1, _ = h.eval(op["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)


def test_trust_exact_reaches_the_lbfgs_threshold():
    """the TLS problem of tests/test_gpu_optimize.py with method="trust-exact": the threshold that test uses for L-BFGS-B"""
    from grape_jl_amd import grape as G

    def flattop(t, T=5.0, t_rise=0.3):
        if t < t_rise:
            return np.sin(np.pi * t / (2 * t_rise)) ** 2
        if t > T - t_rise:
            return np.sin(np.pi * (t - T) / (2 * t_rise)) ** 2
        return 1.0
    H = G.hamiltonian(np.array([[-0.5, 0], [0, 0.5]]), (np.array([[0, 1], [1, 0]]), lambda t: 0.2 * flattop(t)))
    tlist = np.linspace(0, 5, 501)
    traj = G.Trajectory(np.array([1, 0], complex), H, target_state=np.array([0, 1], complex))
    res = G.optimize([traj], tlist, J_T=G.J_T_sm, iter_stop=20, method="trust-exact", rethrow_exceptions=True)
    print(res.J_T, res.message, res.iter)
    assert not res.message.startswith("Exception"), res.message
    assert res.J_T < 1e-3
