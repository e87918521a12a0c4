"""The widened drop-in boundary (ABI v4), through the C ABI on an MI355X:

* ``grape_backward_chi``: a user-defined ``J_T`` / ``chi`` pair (the reference accepts any ``chi(Psi, trajectories;
  tau)``, /root/reference/src/optimize.jl:845-855, src/workspace.jl:306-308) with boundary states that are NOT
  proportional to the targets;
* ``grape_problem.ndev`` / ``devices``: several device shards behind one handle ("multi-GPU is internal to a
  handle -- the caller never sees it").  The box has one GPU, so the shards share it (``devices = [0, 0, ...]``): the
  logic (partition, the two reductions and their order, getters) is the multi-GPU one.
* box bounds through the HIP backend (test/test_tls_optimization.jl:236-263).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def tol_G(Gref):
    return 1e-10 * max(np.abs(Gref).max(), 1e-3)


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    return mod


def observable_functional(N, K, seed):
    """J_T = sum_k w_k <Psi_k(T)|O_k|Psi_k(T)> with Hermitian O_k: chi_k = -dJ_T/d<Psi_k| = -w_k O_k Psi_k(T)."""
    rng = np.random.default_rng(seed)
    O = rng.standard_normal((K, N, N)) + 1j * rng.standard_normal((K, N, N))
    O = (O + np.swapaxes(O.conj(), 1, 2)) / (2 * np.sqrt(N))
    w = 0.5 + rng.random(K)

    def J_T(Psi, trajectories=None, tau=None):
        return float(sum(w[k] * np.real(np.vdot(Psi[k], O[k] @ Psi[k])) for k in range(K)))

    def chi(Psi, trajectories=None, tau=None):
        return [-w[k] * (O[k] @ Psi[k]) for k in range(K)]

    return J_T, chi


@pytest.mark.parametrize("N,L,K,N_T,herm,method,prop", [
    (6, 2, 3, 7, True, 0, 0), (16, 1, 2, 9, False, 1, 0), (40, 2, 3, 5, True, 0, 0), (64, 2, 4, 6, True, 0, 0),
    (64, 2, 4, 6, True, 0, 1), (100, 2, 2, 4, True, 0, 0)])
def test_user_supplied_chi_matches_oracle_and_finite_differences(g, ref, N, L, K, N_T, herm, method, prop):
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=1234 + N, hermitian=herm)
    J_T, chi = observable_functional(N, K, seed=N)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"])
    x = pr["pulsevals"]
    with g.GrapeHip(*args, gradient_method=method, prop_method=prop) as h:
        tau = h.forward(x)
        psiT = h.final_states()
        G = h.backward_chi(np.stack(chi(psiT)))
        tg = h.tau_grads()
        bw = h.storage(1)

        def J_of(xx):
            h.forward(xx)
            return J_T(h.final_states())
        eps = 1e-6
        for idx in (0, L * N_T - 1, (L * N_T) // 2):
            xp, xm = x.copy(), x.copy()
            xp[idx] += eps
            xm[idx] -= eps
            fd = (J_of(xp) - J_of(xm)) / (2 * eps)
            assert abs(fd - G[idx]) <= 2e-8 * max(1.0, abs(G[idx])), (idx, fd, G[idx])
        # the built-in path still works on the same handle afterwards (the custom sweep overwrote the backward states)
        J1, G1, _ = h.eval(x)
    Jr, Gr, _ = ref.evaluate(*args[:3], x, *args[3:], None, gradient_method=method)
    assert abs(J1 - Jr) <= 1e-12 and np.abs(G1 - Gr).max() <= tol_G(Gr)
    # oracle with the same boundary states (computed from ITS final states)
    _, _, taur, parts = ref.evaluate(*args[:3], x, *args[3:], None, gradient=False, want_parts=True)
    Gc, tauc, psiTc, tgc = ref.evaluate_chi(*args[:3], x, *args[3:], np.stack(chi(parts["psiT"])), gradient_method=method)
    assert np.abs(tau - tauc).max() <= 1e-12 and np.abs(psiT - psiTc).max() <= 1e-12
    assert np.abs(G - Gc).max() <= tol_G(Gc)
    assert np.abs(tg - tgc).max() <= 1e-10 * max(np.abs(tgc).max(), 1e-3)
    # backward states are the normalised chi (optimize.jl:867-868)
    c0 = np.stack(chi(psiT))
    assert np.abs(bw[:, -1] - c0 / np.linalg.norm(c0, axis=1, keepdims=True)).max() <= 1e-13


def test_user_supplied_chi_with_state_running_cost_and_zero_norm_guard(g, ref):
    from grape_jl_amd import synth
    N, L, K, N_T = 16, 2, 3, 6
    pr = synth.make_problem(N, L, N_T, K, seed=77)
    J_T, chi = observable_functional(N, K, seed=3)
    rng = np.random.default_rng(0)
    D = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    D = (D + D.conj().T) / 4
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"])
    with g.GrapeHip(*args, D=D, lambda_b=0.3) as h:
        h.forward(pr["pulsevals"])
        psiT = h.final_states()
        G = h.backward_chi(np.stack(chi(psiT)))
        Jb = h.sums()[4]
        # chi = 0 for one trajectory and no running cost to lift it: the guard of optimize.jl:1021-1025
    _, _, _, parts = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], None, gradient=False, want_parts=True, D=D, lambda_b=0.3)
    Gc, *_ = ref.evaluate_chi(*args[:3], pr["pulsevals"], *args[3:], np.stack(chi(parts["psiT"])), D=D, lambda_b=0.3)
    assert np.abs(G - Gc).max() <= tol_G(Gc)
    Jfull, _, _ = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], None, gradient=False, D=D, lambda_b=1.0)
    J0, _, _ = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], None, gradient=False)
    assert abs(Jb - (Jfull - J0)) <= 1e-12
    with g.GrapeHip(*args) as h:
        h.forward(pr["pulsevals"])
        c = np.stack(chi(h.final_states()))
        c[1] = 0.0
        with pytest.raises(g.GrapeHipError) as ei:
            h.backward_chi(c)
        assert ei.value.code == -3


def test_custom_functional_through_the_mirror_optimizes(g):
    """optimize(...; J_T = user function, chi = user function): population transfer with J_T = 1 - |<1|Psi(T)>|^2 written
    as an observable expectation value -- same optimum as J_T_ss, reached through grape_backward_chi."""
    from grape_jl_amd import grape as G
    H = G.hamiltonian(np.array([[-0.5, 0], [0, 0.5]]), (np.array([[0, 1], [1, 0]]), lambda t: 0.2))
    tlist = np.linspace(0, 5, 201)
    traj = G.Trajectory(np.array([1, 0], complex), H, target_state=np.array([0, 1], complex))
    P0 = np.array([[1, 0], [0, 0]], complex)   # population left in |0>

    def J_pop(Psi, trajectories, tau=None):
        return float(np.real(np.vdot(Psi[0], P0 @ Psi[0])))

    def chi_pop(Psi, trajectories, tau=None):
        return [-(P0 @ Psi[0])]
    res = G.optimize([traj], tlist, J_T=J_pop, chi=chi_pop, iter_stop=8)
    assert res.J_T < 1e-3, res
    ref_res = G.optimize([traj], tlist, J_T=G.J_T_ss, iter_stop=8)
    assert ref_res.J_T < 1e-3
    with pytest.raises(ValueError):
        G.optimize([traj], tlist, J_T=J_pop, iter_stop=1)   # a user J_T without its chi


@pytest.mark.parametrize("N,L,K,N_T,functional,ndev,with_d", [
    (6, 2, 5, 7, 0, 2, False), (16, 1, 7, 5, 1, 3, False), (64, 2, 9, 6, 0, 4, False), (64, 2, 6, 5, 2, 8, True),
    (100, 2, 4, 3, 0, 2, False)])
def test_device_shards_behind_one_handle(g, ref, N, L, K, N_T, functional, ndev, with_d):
    """grape_problem.ndev > 1 (shards share the box's one GPU): identical to the single-device handle up to the order
    of the sum over k (<= 1e-13 relative), and to the oracle within the stated tolerance; ndev = 1 is today's handle."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=4321 + N)
    pr["weights"] = 0.5 + np.arange(K) / K
    rng = np.random.default_rng(1)
    D = None
    if with_d:
        D = rng.standard_normal((K, N, N)) + 1j * rng.standard_normal((K, N, N))
        D = (D + np.swapaxes(D.conj(), 1, 2)) / 4
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    kw = dict(functional=functional, D=D, lambda_b=0.4 if with_d else 0.0)
    x = pr["pulsevals"]
    with g.GrapeHip(*args, **kw) as h1:
        J1, G1, tau1, psi1 = h1.eval(x, want_psiT=True)
        tg1, fw1, w1 = h1.tau_grads(), h1.storage(0), h1.work()
        U1 = h1.propagator(K - 1, N_T - 1)
    with g.GrapeHip(*args, devices=[0] * ndev, **kw) as hm:
        Jm, Gm, taum, psim = hm.eval(x, want_psiT=True)
        assert abs(Jm - J1) <= 1e-14 and np.array_equal(taum, tau1) and np.array_equal(psim, psi1)
        assert np.abs(Gm - G1).max() <= 1e-13 * max(np.abs(G1).max(), 1e-3)
        assert np.abs(hm.tau_grads() - tg1).max() <= 1e-13 * max(np.abs(tg1).max(), 1e-3)
        assert np.array_equal(hm.storage(0), fw1)
        assert np.array_equal(hm.propagator(K - 1, N_T - 1), U1)
        wm = hm.work()
        assert wm["cells"] == w1["cells"] and abs(wm["flop_expm"] - w1["flop_expm"]) <= 1e-12 * w1["flop_expm"]
        Jf, Gf, _ = hm.eval(x, gradient=False)
        assert Gf is None and Jf == Jm
        J2, G2, _ = hm.eval(x)
        assert J2 == Jm and np.array_equal(G2, Gm)      # fixed reduction order: bitwise repeatable
        assert hm.timings()["expm"] > 0
        # split-phase calls on the composite (it may itself be a shard of a larger job) and the custom-chi route
        taus = hm.forward(x)
        s = hm.sums()
        assert np.array_equal(taus, tau1)
        Gs = hm.backward(complex(s[0], s[1]))
        assert np.array_equal(Gs, Gm)
        if not with_d and N <= 64:
            c = np.conj(pr["target"]) * (1.0 + np.arange(K))[:, None]
            Gc = hm.backward_chi(c)
            h1b = g.GrapeHip(*args, **kw)
            h1b.forward(x)
            assert np.abs(Gc - h1b.backward_chi(c)).max() <= 1e-13 * max(np.abs(Gc).max(), 1e-3)
            h1b.close()
        # device-pointer entry points are single-device only: loud refusal, not silent misuse
        with pytest.raises(g.GrapeHipError):
            hm.forward_device(0, 0, 0)
    Jr, Gr, taur = ref.evaluate(*args[:3], x, *args[3:], functional=functional, **(dict(D=D, lambda_b=0.4) if with_d else {}))
    assert abs(Jm - Jr) <= 1e-12 and np.abs(taum - taur).max() <= 1e-12 and np.abs(Gm - Gr).max() <= tol_G(Gr)


def test_more_devices_than_trajectories_and_bad_ordinal(g):
    from grape_jl_amd import synth
    pr = synth.make_problem(6, 1, 4, 2, seed=9)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"])
    with g.GrapeHip(*args) as h1, g.GrapeHip(*args, devices=[0, 0, 0, 0]) as hm:   # 2 trajectories -> 2 shards
        J1, G1, _ = h1.eval(pr["pulsevals"])
        Jm, Gm, _ = hm.eval(pr["pulsevals"])
        assert abs(J1 - Jm) <= 1e-15 and np.abs(G1 - Gm).max() <= 1e-15
    with pytest.raises(g.GrapeHipError) as ei:
        g.GrapeHip(*args, devices=[0, 99])
    assert ei.value.code == -2 and "device shard 1" in str(ei.value)
    # the failed create leaves no sticky HIP error behind: the next evaluation of a healthy handle works
    with g.GrapeHip(*args) as h1:
        J2, G2, _ = h1.eval(pr["pulsevals"])
    assert J2 == J1 and np.array_equal(G2, G1)


def test_box_bounds_through_the_hip_backend(g):
    # /root/reference/test/test_tls_optimization.jl:236-263 (thresholds as there)
    from grape_jl_amd import grape as G
    H = G.hamiltonian(np.array([[-0.5, 0], [0, 0.5]]), (np.array([[0, 1], [1, 0]]), lambda t: 0.2))
    tlist = np.linspace(0, 5, 501)
    traj = G.Trajectory(np.array([1, 0], complex), H, target_state=np.array([0, 1], complex))
    res = G.optimize([traj], tlist, J_T=G.J_T_sm, iter_stop=10, upper_bound=0.7, lower_bound=-0.7,
                     check_convergence=lambda r: "J_T < 10^-10" if r.J_T < 1e-10 else "")
    assert not res.message.startswith("Exception"), res.message
    assert res.J_T < 1e-3
    assert 0.65 < np.max(np.abs(res.optimized_controls[0])) < 0.700001
    # per-control bounds with the reference's pulse_options keys (workspace.jl:204-214); L = 1: both layouts coincide
    ctrl = traj.generator.controls[0]
    res2 = G.optimize([traj], tlist, J_T=G.J_T_sm, iter_stop=10,
                      pulse_options=[(ctrl, {"upper_bounds": 0.6, "lower_bounds": -0.6})])
    assert res2.J_T < 1e-2 and np.max(np.abs(res2.optimized_controls[0])) < 0.600001


def test_blocked_path_squaring_plan_without_host_synchronisation(g, ref):
    """64 < N <= 256: the squaring count of scaling and squaring is only known on the device; the host issues a plan of
    launches that exit when they are not needed instead of reading the count back between launches (no
    hipStreamSynchronize inside grape_forward_device).  A plan that is too short flags the evaluation: the host-pointer
    calls repeat internally (results identical to the oracle), the device-pointer call reports GRAPE_ERR_AGAIN once and
    succeeds on the repeat."""
    import torch
    from grape_jl_amd import synth
    from grape_jl_amd.sharded import ShardedEvaluator
    # ||A||_1 ~ 62 (Julia's exp! would square 4 times), spectral bound ~ 15: the polynomial route squares 3 times, more
    # than the initial plan of 2 launches
    pr = synth.make_problem(100, 1, 3, 2, seed=5, dt=12.0)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    x = pr["pulsevals"]
    Jr, Gr, taur = ref.evaluate(*args[:3], x, *args[3:])
    with g.GrapeHip(*args) as h:
        J, G, tau = h.eval(x)                     # plan too short -> adapted -> repeated inside grape_forward
        w = h.work()
        assert w["squarings"] / w["cells"] >= 3 and w["t18_squarings"] / w["t18_cells"] >= 3
        # (the oracle's own rounding grows with the norm of the step)
        assert abs(J - Jr) <= 1e-11 and np.abs(tau - taur).max() <= 1e-11 and np.abs(G - Gr).max() <= 10 * tol_G(Gr)
        J2, G2, _ = h.eval(x)                     # the adapted plan fits: same numbers
        assert J2 == J and np.array_equal(G2, G)
    with g.GrapeHip(*args) as h:                  # fresh handle, device-pointer API
        dev = torch.device("cuda", 0)
        ev = ShardedEvaluator(h, 2, g.J_T_SM, dist=None, device=dev)
        xd, out, Gd = ev.alloc_device(1, 3, 2)
        xd.copy_(torch.from_numpy(x))
        stream = torch.cuda.current_stream(dev).cuda_stream
        ev.eval_device(stream)
        with pytest.raises(g.GrapeHipError) as ei:
            h.check(stream)
        assert ei.value.code == -7
        ev.eval_device(stream)
        h.check(stream)
        assert ev.J_device() == J and np.array_equal(Gd.cpu().numpy(), G)
    # composite handle: every shard adapts its own plan, one internal repeat
    with g.GrapeHip(*args, devices=[0, 0]) as hm:
        Jm, Gm, _ = hm.eval(x)
        assert abs(Jm - J) <= 1e-14 and np.abs(Gm - G).max() <= 1e-13 * max(np.abs(G).max(), 1e-3)


@pytest.mark.parametrize("prop", [0, 1], ids=["coop_sweeps", "cheby_sweeps"])
def test_cooperative_kernels_time_out_instead_of_hanging(g, prop, monkeypatch):
    """The cooperative kernels (sweep_coop_kernel for ExpProp at N > 64, cheby_coop_kernel for the polynomial propagator)
    let several workgroups share a trajectory and wait for each other.  Fault injection: one sibling of every trajectory
    exits at once (GRAPE_TEST_DROP_SIBLING).  The others must run into their bounded spin, raise flag 8 and let the grid
    drain: the call fails with GRAPE_ERR_HIP within seconds, and the same handle evaluates correctly afterwards."""
    import time
    from grape_jl_amd import synth
    pr = synth.make_problem(100, 1, 4, 2, seed=12)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"])
    monkeypatch.setenv("GRAPE_TEST_HOOKS", "1")   # (read at grape_create: only then is the fault switch looked up per evaluation)
    with g.GrapeHip(*args, prop_method=prop) as h:
        J0, G0, _ = h.eval(pr["pulsevals"])
        monkeypatch.setenv("GRAPE_TEST_DROP_SIBLING", "2")
        t0 = time.time()
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval(pr["pulsevals"])
        assert ei.value.code == -2 and "sibling" in str(ei.value)
        assert time.time() - t0 < 60.0
        monkeypatch.delenv("GRAPE_TEST_DROP_SIBLING")
        J1, G1, _ = h.eval(pr["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)


def test_arbitrary_state_running_cost_through_xi(g):
    """ABI v5, grape_backward_xi: an ARBITRARY g_b (optimize.jl:727-750, 856-866, 897-908).  The reference calls the user's
    g_b / xi inside its loops; here the forward sweep runs on the device, the caller evaluates xi_k(t_n) on the stored
    states and the backward sweep takes the array.  g_b = <Psi|D|Psi>^2 (not of the built-in quadratic family), with the
    built-in J_T_sm and with a user-supplied chi, against the numpy oracle with the same callbacks and against central
    finite differences of the total functional; the concurrent sweeps are switched off and ONE backward sweep runs."""
    import grape_oracle as go
    from grape_jl_amd import synth
    N, L, N_T, K = 12, 2, 7, 3
    pr = synth.make_problem(N, L, N_T, K, seed=91)
    rng = np.random.default_rng(3)
    D = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    D = (D + D.conj().T) / 4
    lam = 0.7
    g_b = lambda psi, k, n: float(np.real(np.vdot(psi, D @ psi))) ** 2                     # noqa: E731
    xi = lambda psi, k, n: -2.0 * float(np.real(np.vdot(psi, D @ psi))) * (D @ psi)        # noqa: E731  -d g_b / d<Psi|
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    x = pr["pulsevals"]
    tl = pr["tlist"]

    def total(h, xx):
        h.forward(xx)
        fw = h.storage(0)
        Jb = 0.0
        for k in range(K):
            Jb += g_b(fw[k, 0], k, 0) * (tl[1] - tl[0]) / 2
            for n in range(1, N_T + 1):
                dt = 0.5 * (tl[n + 1] - tl[n - 1]) if n < N_T else (tl[-1] - tl[-2]) / 2
                Jb += g_b(fw[k, n], k, n) * dt
        sm = h.sums()
        return 1.0 - (sm[0] ** 2 + sm[1] ** 2) / K ** 2 + lam * Jb, fw

    with g.GrapeHip(*args) as h:
        assert h.set_fused_sweeps(False) is False
        J, fw = total(h, x)
        h.reset_timings()
        xi_arr = np.zeros_like(fw)
        for k in range(K):
            for n in range(1, N_T + 1):
                xi_arr[k, n] = xi(fw[k, n], k, n)
        G = h.backward_xi(xi_arr, lam)
        Jr, Gr, _ = go.evaluate_gradient(*args[:3], x, *args[3:], lambda_b=lam, g_b=g_b, xi=xi)
        assert abs(J - Jr) <= 1e-12 and np.abs(G - Gr).max() <= 1e-10 * max(np.abs(Gr).max(), 1e-3)
        for i in (0, 5, L * N_T - 1):                       # finite differences of the GPU functional itself
            e = np.zeros_like(x); e[i] = 1e-6
            fd = (total(h, x + e)[0] - total(h, x - e)[0]) / 2e-6
            assert abs(fd - G[i]) <= 2e-8 * max(1.0, abs(G[i]))
        # with a caller-supplied chi as well (chi of J_T_sm written out by hand)
        tau = h.forward(x)
        chi = (np.sum(pr["weights"] * tau) / K ** 2) * pr["weights"][:, None] * pr["target"]
        G2 = h.backward_xi(xi_arr, lam, chi=chi)
        assert np.abs(G2 - G).max() <= 1e-13 * max(np.abs(G).max(), 1e-3)


def test_custom_chi_route_runs_one_backward_sweep(g):
    """The mirror's custom-chi backend (and julia/GrapeHIP.jl make_fg! for functional_code == -1) switches the concurrent
    sweeps off: the forward call of the custom route must not pay for a unit-target backward sweep that grape_backward_chi
    then repeats.  HIP-event timings: the forward phase of the custom route costs what a forward-only evaluation costs."""
    import grape_jl_amd.grape as gm
    from grape_jl_amd import synth
    N, L, N_T, K = 64, 1, 400, 64
    pr = synth.make_problem(N, L, N_T, K, seed=17)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    chi_fn = lambda psis, trajs, tau=None: [  # noqa: E731  (chi of J_T_sm)
        (np.sum(np.asarray(tau)) / K ** 2) * pr["target"][k] for k in range(K)]
    J_fn = lambda psis, trajs, tau=None: 1.0 - abs(np.sum(np.asarray(tau))) ** 2 / K ** 2   # noqa: E731
    with g.GrapeHip(*args) as inner:
        be = gm._CustomChiBackend(inner, J_fn, chi_fn, [None] * K)
        be.eval(pr["pulsevals"])
        inner.reset_timings()
        J, G, tau = be.eval(pr["pulsevals"])
        t_custom = inner.timings()
        inner.reset_timings()
        inner.eval(pr["pulsevals"], gradient=False)
        t_fwd = inner.timings()
    with g.GrapeHip(*args) as h:
        Jb, Gb, _ = h.eval(pr["pulsevals"])
    assert abs(J - Jb) <= 1e-12 and np.abs(G - Gb).max() <= 1e-10 * max(np.abs(Gb).max(), 1e-3)
    # forward sweep alone in both cases (a fused launch of both directions takes visibly longer: 2K workgroups share HBM)
    assert t_custom["forward"] <= 1.25 * t_fwd["forward"] + 0.05


def test_composite_handle_reduces_with_rccl(g, monkeypatch):
    """Several devices behind one handle: the two cross-shard reductions are RCCL all-reduces on the shard streams when every
    shard has a device of its own (north_star: "an RCCL all-reduce of the gradient vector over xGMI").  This box has ONE GPU:
    GRAPE_MULTI_RCCL=1 with devices = [0] builds the composite handle with one shard behind a one-rank communicator -- the
    whole collective code path (ncclCommInitAll, grouped ncclAllReduce of the 8 sums and of the gradient, totals read back
    from the first shard) -- and must reproduce the plain handle bit for bit.  Repeated ordinals stay host-staged."""
    from grape_jl_amd import synth
    pr = synth.make_problem(24, 2, 12, 5, seed=44)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args) as h:
        J0, G0, tau0 = h.eval(pr["pulsevals"])
    monkeypatch.setenv("GRAPE_MULTI_RCCL", "1")
    with g.GrapeHip(*args, devices=[0]) as h:
        J1, G1, tau1 = h.eval(pr["pulsevals"])
        J2, G2, tau2 = h.eval(pr["pulsevals"])
        tm = h.timings()
        sums = h.sums() if hasattr(h, "sums") else None
    monkeypatch.delenv("GRAPE_MULTI_RCCL")
    if "gradient_allreduce_us" not in tm:
        pytest.skip("RCCL could not be loaded / initialised on this box: the composite handle fell back to host staging")
    assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(tau1, tau0)
    assert J2 == J0 and np.array_equal(G2, G0)
    assert tm["gradient_allreduce_us"] > 0.0
    with g.GrapeHip(*args, devices=[0, 0]) as h:          # two shards on one ordinal: host-staged, in shard order
        J3, G3, _ = h.eval(pr["pulsevals"])
        assert "gradient_allreduce_us" not in h.timings()
    assert abs(J3 - J0) <= 1e-13 and np.abs(G3 - G0).max() <= 1e-13 * max(np.abs(G0).max(), 1e-3)


# ---- ABI v6 (round 5) ----
def test_trajectories_without_target_states(g, ref):
    """grape_problem.target == NULL (optimize.jl:753: tau_k = NaN, legal with a user-defined J_T): the caller-side route
    forward + final_states + backward_chi works and equals the oracle's; everything that needs a target refuses loudly."""
    from grape_jl_amd import synth
    for N, L, K, N_T, herm in [(6, 2, 3, 7, True), (64, 2, 4, 6, True), (20, 1, 2, 9, False), (100, 2, 2, 4, True)]:
        pr = synth.make_problem(N, L, N_T, K, seed=4321 + N, hermitian=herm)
        J_T, chi = observable_functional(N, K, seed=N)
        x = pr["pulsevals"]
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], None) as h:
            tau = h.forward(x)
            assert np.isnan(tau).all()
            assert np.isnan(h.sums()[:4]).all()
            psiT = h.final_states()
            G = h.backward_chi(np.stack(chi(psiT)))
            for call in (lambda: h.eval(x), lambda: h.backward(1.0 + 0j)):
                with pytest.raises(g.GrapeHipError) as ei:
                    call()
                assert ei.value.code == -1 and "target" in str(ei.value)
        args = (pr["H0"], pr["Hc"], pr["tlist"])
        _, _, _, parts = ref.evaluate(*args, x, pr["psi0"], pr["target"], None, gradient=False, want_parts=True)
        Gc, _, psiTc, _ = ref.evaluate_chi(*args, x, pr["psi0"], pr["target"], np.stack(chi(parts["psiT"])))
        assert np.abs(psiT - psiTc).max() <= 1e-12
        assert np.abs(G - Gc).max() <= tol_G(Gc)


def test_custom_functional_without_targets_through_the_mirror(g):
    """Trajectory(initial_state, generator) without target_state + user J_T / chi: the mirror hands no target array over"""
    from grape_jl_amd import grape as G
    H = G.hamiltonian(np.array([[-0.5, 0], [0, 0.5]]), (np.array([[0, 1], [1, 0]]), lambda t: 0.2))
    tlist = np.linspace(0, 5, 201)
    traj = G.Trajectory(np.array([1, 0], complex), H)
    P0 = np.array([[1, 0], [0, 0]], complex)
    res = G.optimize([traj], tlist, J_T=lambda Psi, tr, tau=None: float(np.real(np.vdot(Psi[0], P0 @ Psi[0]))),
                     chi=lambda Psi, tr, tau=None: [-(P0 @ Psi[0])], iter_stop=8)
    assert res.J_T < 1e-3, res
    assert np.isnan(res.tau_vals).all()


@pytest.mark.parametrize("N,L,K,N_T", [(10, 1, 2, 6), (24, 2, 3, 8), (64, 2, 2, 5), (48, 1, 2, 5)])
def test_taylor_grad_check_convergence_false(g, ref, N, L, K, N_T):
    """taylor_grad_check_convergence = false (optimize.jl:917-918, taylor_grad_step! :631-651): a series cut at
    taylor_grad_max_order is not an error and the truncated sum is what the reference returns -- against the C restatement
    with the same three settings.  With the check on the same call raises, as the reference does (:644-648)."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=99 + N)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    x = pr["pulsevals"]
    try:
        for order in (6, 40):      # 6: every series is cut (||H dt|| ~ 1 needs ~19 terms); 40: none is
            ref.set_taylor(order, 1e-16, False)
            Jr, Gr, _ = ref.evaluate(*args[:3], x, *args[3:], gradient_method=1)
            with g.GrapeHip(*args, gradient_method=g.GRAD_TAYLOR, taylor_max_order=order, taylor_check_convergence=False) as h:
                J, G, _ = h.eval(x)
            assert abs(J - Jr) <= 1e-12
            assert np.abs(G - Gr).max() <= tol_G(Gr), (order, np.abs(G - Gr).max())
        ref.set_taylor()
        _, Gfull, _ = ref.evaluate(*args[:3], x, *args[3:], gradient_method=1)
        assert np.abs(Gr - Gfull).max() <= tol_G(Gfull)             # 40 terms had converged
        ref.set_taylor(6, 1e-16, False)
        _, G6, _ = ref.evaluate(*args[:3], x, *args[3:], gradient_method=1)
        assert np.abs(G6 - Gfull).max() > 1e3 * tol_G(Gfull)        # ... and 6 had not: the test above pinned a truncated sum
    finally:
        ref.set_taylor()
    with g.GrapeHip(*args, gradient_method=g.GRAD_TAYLOR, taylor_max_order=6) as h:
        with pytest.raises(g.GrapeHipError, match="GRAPE_ERR_TAYLOR"):
            h.eval(x)


def test_exception_barrier_with_device_memory_in_flight(g, monkeypatch):
    """a C++ exception at the END of grape_create -- the handle owns its device buffers, streams and events by then --
    comes back as GRAPE_ERR_HOST and leaks nothing: free device memory returns to where it was, and the next create works"""
    import torch
    from grape_jl_amd import synth
    pr = synth.make_problem(64, 2, 200, 16, seed=8)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args) as h:                       # (runtime warm: module loads, pools)
        h.eval(pr["pulsevals"])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    monkeypatch.setenv("GRAPE_TEST_HOOKS", "1")
    monkeypatch.setenv("GRAPE_TEST_THROW_AT", "late")
    monkeypatch.setenv("GRAPE_TEST_THROW", "bad_alloc")
    for devices in (None, [0, 0]):                     # plain handle; composite handle (the second shard's create throws too)
        with pytest.raises(g.GrapeHipError) as ei:
            g.GrapeHip(*args, devices=devices)
        assert ei.value.code == -8 and "bad_alloc" in str(ei.value)
    monkeypatch.delenv("GRAPE_TEST_HOOKS")
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 64 << 20      # 16 x 200 propagators alone are 210 MB
    with g.GrapeHip(*args) as h:
        J, G, _ = h.eval(pr["pulsevals"])
        assert np.isfinite(J) and np.isfinite(G).all()


def _cycle_closed_batch(g):
    """N = 16 on the batched route: 4 sets, then 8 (release and regrow); the propagators alone are 13 MB per set"""
    from grape_jl_amd import synth
    pr = synth.make_problem(16, 2, 400, 8, seed=21)
    X = np.stack([s * pr["pulsevals"] for s in (1.0, 0.5, 1.3, 0.7, 0.9, 1.1, 0.6, 1.2)])

    def cycle():
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"]) as h:
            for P in (4, 8):
                J, G, _ = h.eval_batch(X[:P])
                assert h.batch_info()["route"] == 1 and h.batch_info()["sets_per_group"] == P
                assert np.isfinite(J).all() and np.isfinite(G).all() and np.abs(G).max() > 0
    return cycle


def _cycle_closed_hvp(g):
    """N = 64: 4 directions, then 8 (5.5 MB each), and the buffers of the first time gradient and the first caller's chi"""
    from grape_jl_amd import synth
    pr = synth.make_problem(64, 2, 200, 16, seed=8)
    x = pr["pulsevals"]
    V = np.random.default_rng(5).standard_normal((8, x.size))

    def cycle():
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"]) as h:
            J, G, _ = h.eval(x)
            outs = [G, h.hvp(V[:4]), h.hvp(V), h.time_gradient(), h.backward_chi(0.25 * np.conj(h.final_states()))]
            assert h.hvp_info()["dirs_per_group"] == 8 and h.hvp_info()["bytes"] > 8 * (5 << 20)
            assert np.isfinite(J) and all(np.isfinite(o).all() and np.abs(o).max() > 0 for o in outs)
    return cycle


def _cycle_open(g):
    """d = 32, J = 2: 8 directions (3 MB each), 8 then 16 pulse sets (2.4 MB each), time gradient, a caller's chi"""
    from grape_jl_amd import synth
    pr = synth.make_open_problem(32, 2, 50, 2, 2, seed=3202)
    x = pr["pulsevals"]
    V = np.random.default_rng(6).standard_normal((8, x.size))
    X = np.stack([(0.5 + 0.05 * p) * x for p in range(16)])

    def cycle():
        with g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr["target"]) as h:
            J, G, _ = h.eval(x)
            outs = [G, h.open_hvp(V)]
            for P in (8, 16):
                Jb, Gb, _ = h.open_eval_batch(X[:P])
                assert h.open_batch_info()["sets_per_group"] == P
                outs += [Jb, Gb]
            outs += [h.time_gradient(), h.backward_chi(0.25 * pr["target"])]
            assert h.open_hvp_info()["bytes"] > 8 * (2 << 20) and h.open_batch_info()["bytes"] > 16 * (2 << 20)
            assert np.isfinite(J) and all(np.isfinite(o).all() and np.abs(o).max() > 0 for o in outs)
    return cycle


@pytest.mark.parametrize("which", ["closed_batch", "closed_hvp", "open"])
def test_create_use_every_growing_store_destroy_repeatedly(g, monkeypatch, which):
    """whatever a handle allocated -- the buffers of grape_create, the storage of grape_eval_batch, grape_hvp, grape_open_hvp and
    grape_open_eval_batch after it has grown once, the buffers of the first time gradient and of the first caller's chi --
    goes with the handle: after eight create / use / destroy cycles free device memory is where it was (64 MB of slack, as
    above; one leaked store would be 190 MB or more)"""
    import torch
    monkeypatch.setenv("GRAPE_BATCH", "1")
    cycle = {"closed_batch": _cycle_closed_batch, "closed_hvp": _cycle_closed_hvp, "open": _cycle_open}[which](g)
    cycle()                                            # (runtime warm: module loads, pools)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(8):
        cycle()
    torch.cuda.synchronize()
    drift = torch.cuda.mem_get_info()[0] - free0
    print(dict(which=which, drift_mb=drift / 2 ** 20))
    assert abs(drift) <= 64 << 20


def test_composite_handle_validates_its_first_collective(g, monkeypatch):
    """the first evaluation of a handle that reduces with RCCL also takes the host-staged sums and compares (advisor
    finding of round 4: the collective path had never been checked against anything); a second handle on the same device
    list reuses the cached communicator set"""
    import time
    from grape_jl_amd import synth
    pr = synth.make_problem(16, 1, 10, 4, seed=2)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    monkeypatch.setenv("GRAPE_MULTI_RCCL", "1")
    t0 = time.perf_counter()
    with g.GrapeHip(*args, devices=[0]) as h:
        J1, G1, _ = h.eval(pr["pulsevals"])
        rccl = "gradient_allreduce_us" in h.timings()
    t1 = time.perf_counter()
    with g.GrapeHip(*args, devices=[0]) as h:
        J2, G2, _ = h.eval(pr["pulsevals"])
    t2 = time.perf_counter()
    if not rccl:
        pytest.skip("RCCL could not be loaded / initialised on this box")
    assert J1 == J2 and np.array_equal(G1, G2)
    if (t1 - t0) > 0.05:                                 # (the first handle really initialised a communicator set: tens of ms; an
        assert (t2 - t1) < (t1 - t0)                     #  earlier test of this process may have left it in the cache) -- no second one


@pytest.mark.parametrize("N,L,N_T,K,kw", [(16, 1, 50, 8, {}), (64, 2, 30, 128, {}), (40, 2, 20, 3, {"functional": 1}),
                                          (24, 2, 16, 4, {"prop_method": 1}), (64, 2, 12, 5, {"gradient_method": 1})])
def test_captured_graph_replays_the_evaluation_bit_for_bit(g, monkeypatch, N, L, N_T, K, kw):
    """grape_eval with a gradient replays the whole evaluation as one captured HIP graph from its third call on (N <= 64, one
    device; every 16th call and the two behind a grape_reset_timings run uncaptured).  Twenty evaluations with fresh pulses
    each: identical, bit for bit, to the same calls with GRAPE_GRAPH=0; switching the concurrent sweeps off rebuilds the
    graph; the error flags of a replayed evaluation still surface; the phase timings stay alive."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=17 + N)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    rng = np.random.default_rng(0)
    xs = [pr["pulsevals"] + 1e-2 * rng.standard_normal(L * N_T) for _ in range(20)]
    out = {}
    for graph in ("1", "0"):
        monkeypatch.setenv("GRAPE_GRAPH", graph)
        with g.GrapeHip(*args, **kw) as h:
            res = [h.eval(x) for x in xs[:12]]
            assert h.set_fused_sweeps(False) is False
            res += [h.eval(x) for x in xs[12:16]]
            h.set_fused_sweeps(True)
            h.reset_timings()
            res += [h.eval(x) for x in xs[16:]]
            tm = h.timings()
            assert tm["expm"] > 0 or kw.get("prop_method") == 1
            assert tm["total"] > 0
            fw = h.storage(0)
            out[graph] = (res, fw)
    for (Ja, Ga, ta), (Jb, Gb, tb) in zip(out["1"][0], out["0"][0]):
        assert Ja == Jb and np.array_equal(Ga, Gb) and np.array_equal(ta, tb)
    assert np.array_equal(out["1"][1], out["0"][1])
    monkeypatch.setenv("GRAPE_GRAPH", "1")
    with g.GrapeHip(*args, chi_min_norm=1e3, **kw) as h:      # the chi-norm guard fires in every evaluation, replayed or not
        for x in xs[:6]:
            with pytest.raises(g.GrapeHipError) as ei:
                h.eval(x)
            assert ei.value.code == -3


def test_exception_inside_a_shard_thread_stops_at_the_barrier(g, monkeypatch):
    """round-5 advisor finding: the exception barrier of the entry points did not cover WORKER threads -- a std::bad_alloc
    inside a shard's enqueue thread (or inside a parallel_for worker of grape_create) left the thread function and ended
    the process in std::terminate.  Injected here in the last shard's thread of a composite handle's evaluation and in a
    worker of grape_create: both come back as GRAPE_ERR_HOST with a message, the process lives, the next call works."""
    from grape_jl_amd import synth
    pr = synth.make_problem(24, 2, 12, 6, seed=19)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    monkeypatch.setenv("GRAPE_TEST_HOOKS", "1")
    monkeypatch.setenv("GRAPE_TEST_THROW_AT", "none")
    monkeypatch.setenv("GRAPE_TEST_THROW", "bad_alloc")
    with g.GrapeHip(*args, devices=[0, 0, 0]) as h:           # three shards on this box's one GPU, one host thread each
        J0, G0, _ = h.eval(pr["pulsevals"])
        monkeypatch.setenv("GRAPE_TEST_THROW_AT", "shard")
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval(pr["pulsevals"])
        assert ei.value.code == -8 and "bad_alloc" in str(ei.value)
        monkeypatch.setenv("GRAPE_TEST_THROW_AT", "none")
        J1, G1, _ = h.eval(pr["pulsevals"])                   # the handle is still usable
        assert J1 == J0 and np.array_equal(G1, G0)
    # a worker thread of grape_create's host-side set-up (shape factors of the four-product route's plan: parallel_for over
    # the generator classes of a Hermitian problem with 16 < N <= 64)
    prn = synth.make_problem(40, 2, 6, 8, seed=20)
    monkeypatch.setenv("GRAPE_TEST_THROW_AT", "worker")
    monkeypatch.setenv("GRAPE_TEST_THROW", "a worker failed")
    with pytest.raises(g.GrapeHipError) as ei:
        g.GrapeHip(prn["H0"], prn["Hc"], prn["tlist"], prn["psi0"], prn["target"], prn["weights"])
    assert ei.value.code == -8 and "a worker failed" in str(ei.value)
    monkeypatch.delenv("GRAPE_TEST_HOOKS")
    with g.GrapeHip(prn["H0"], prn["Hc"], prn["tlist"], prn["psi0"], prn["target"], prn["weights"]) as h:
        assert np.isfinite(h.eval(prn["pulsevals"])[0])


@pytest.mark.parametrize("N", [16, 40, 64])
def test_gradgen_never_accepts_an_unconverged_series(g, monkeypatch, N):
    """round-5 advisor finding: taylor_grad_check_convergence = false belongs to gradient_method = :taylor
    (optimize.jl:917-918); :gradgen shares the series kernels and their non-convergence flag, and the switch used to
    silence a :gradgen series that had not converged -- a wrong gradient with GRAPE_OK.  A tolerance no term can reach
    forces the non-convergence: :gradgen reports it whatever the switch says."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, 6, 3, seed=5)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    monkeypatch.setenv("GRAPE_GRADGEN_TOL", "0")
    for check in (True, False):
        with g.GrapeHip(*args, gradient_method=g.GRAD_GRADGEN, taylor_check_convergence=check) as h:
            with pytest.raises(g.GrapeHipError) as ei:
                h.eval(pr["pulsevals"])
            assert ei.value.code == -5
    monkeypatch.delenv("GRAPE_GRADGEN_TOL")
    with g.GrapeHip(*args, gradient_method=g.GRAD_GRADGEN, taylor_check_convergence=False) as h:
        assert np.isfinite(h.eval(pr["pulsevals"])[1]).all()


@pytest.mark.parametrize("N,L,K,herm,custom", [(8, 1, 2, True, False), (64, 2, 3, True, False), (20, 2, 2, False, True)])
def test_time_dependent_term_that_is_not_a_control_rides_as_a_pseudo_control(g, ref, N, L, K, herm, custom):
    """A generator term with a time-dependent coefficient that is NOT optimised (an amplitude whose get_controls is empty;
    the reference re-evaluates the generator on every interval, optimize.jl:732, 881, 937-945) crosses the boundary as a
    pseudo-control: extra operator, fixed pulse values, its gradient rows dropped (FixedAmplitude).
    Against the oracle with the drive written out as an (L+1)-th control: J, tau and the L optimised rows of G."""
    from grape_jl_amd import grape as G_, synth
    N_T = 9
    pr = synth.make_problem(N, L + 1, N_T, K, seed=77 + N, hermitian=herm)
    tl = pr["tlist"]
    drive = lambda t: 0.3 * np.cos(0.7 * t) - 0.1                                     # noqa: E731
    x_opt = pr["pulsevals"][:L * N_T].copy()
    ctrls = [x_opt[l * N_T:(l + 1) * N_T].copy() for l in range(L)]
    amp = G_.FixedAmplitude(drive)
    trajs = [G_.Trajectory(pr["psi0"][k], G_.hamiltonian(pr["H0"][k], *[(pr["Hc"][l], ctrls[l]) for l in range(L)],
                                                         (pr["Hc"][L], amp)), target_state=pr["target"][k]) for k in range(K)]
    kw = {}
    if custom:
        J_T, chi = observable_functional(N, K, seed=3)
        kw = dict(J_T=J_T, chi=chi)
    else:
        kw = dict(J_T=G_.J_T_sm)
    wrk = G_.GrapeWrk(trajs, tl, **kw)
    assert wrk.L == L and len(wrk.pulsevals) == L * N_T          # the optimiser sees the L controls only
    Gout = np.zeros(L * N_T)
    J = G_.evaluate_gradient_b(Gout, wrk.pulsevals, wrk)
    x_full = np.concatenate([x_opt, G_.discretize_on_midpoints(drive, tl)])
    if custom:
        psiT = _final_states(ref, pr, tl, x_full)
        Gr, taur, _, _ = ref.evaluate_chi(pr["H0"], pr["Hc"], tl, x_full, pr["psi0"], pr["target"], np.stack(chi(list(psiT))))
        Jr = J_T(list(psiT))
    else:
        Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], tl, x_full, pr["psi0"], pr["target"], None)
    assert abs(J - Jr) <= 1e-12
    assert np.abs(wrk.result.tau_vals - taur).max() <= 1e-12
    assert np.abs(Gout - Gr[:L * N_T]).max() <= tol_G(Gr)
    assert len(Gout) == L * N_T


def _final_states(ref, pr, tl, x):
    _, _, _, parts = ref.evaluate(pr["H0"], pr["Hc"], tl, x, pr["psi0"], pr["target"], None, want_parts=True)
    return parts["psiT"]


@pytest.mark.parametrize("N", [12, 40, 64])
def test_taylor_series_of_one_term_is_returned_as_it_is(g, ref, N):
    """taylor_grad_step! raises only `if check_convergence && max_order > 1` (optimize.jl:644): with taylor_grad_max_order = 1
    the loop `for n = 2:max_order` is empty and the first-order term is the result, whatever check_convergence says
    (round-5 advisor finding: the HIP path raised GRAPE_ERR_TAYLOR)"""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, 5, 2, seed=31 + N, dt=0.05)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    ref.set_taylor(1, 1e-16, True)
    try:
        Jr, Gr, _ = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], gradient_method=ref.TAYLOR)
    finally:
        ref.set_taylor()
    with g.GrapeHip(*args, gradient_method=g.GRAD_TAYLOR, taylor_max_order=1) as h:
        J, G, _ = h.eval(pr["pulsevals"])
    assert abs(J - Jr) <= 1e-12 and np.abs(G - Gr).max() <= tol_G(Gr)
