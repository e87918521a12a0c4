"""grape_hvp on the GPU: exact Hessian-vector products of J (include/grape_hip.h, csrc/grape_hvp.hip.h).

Bar: the project's gradient tolerance applied to H v against tests/hvp_reference.py (proved in tests/test_hvp_reference.py),
    ||dHv||_inf <= 1e-10 * max(||Hv||_inf, 1e-3),
and every case asserts on the reference alone min|tau_k| >= 0.1, ||G||_inf >= 1e-3, ||Hv||_inf >= 1e-3, so that the bound is
relative and never its floor.  Every case has N_T = 4 and K <= 3.  "Bit for bit" is ``np.array_equal``.
"""
import numpy as np
import pytest

import grape_jl_amd as g
import hvp_reference as hr
from grape_jl_amd import synth

pytestmark = pytest.mark.gpu

N_T = 4


def make_case(N, L, K, seed, herm=True, per_traj=False, shape=False, weights=False, nonuniform=False, skew=0, dt=1.0, amp=3.0):
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
    if nonuniform:
        pr["tlist"] = np.concatenate([[0.0], np.cumsum(dt * (0.5 + u[:N_T]))])
    pr["shape"] = 0.5 + 0.5 * u[N_T:N_T + L * N_T].reshape(L, N_T) if shape else None
    # True: drawn; False: ones; None: no weights at all, the handle gets NULL
    pr["weights"] = None if weights is None else 0.5 + u[N_T + L * N_T:] if weights else np.ones(K)
    hr.order_one_targets(pr)
    return pr


def handle(pr, functional, **kw):
    return g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=functional,
                      shape=pr["shape"], **kw)


# every padding and both edges of each; the functionals spread over the paddings
CASES = {
    "N3-L1-sm": dict(N=3, L=1, K=2, f=0),
    "N16-L8-ss": dict(N=16, L=8, K=2, f=1, amp=1.0),
    "N16-L2-re": dict(N=16, L=2, K=2, f=2),
    # weights == NULL in grape_problem: the other arm of every `weights ? weights[k] : 1.0` (sm: coefficient and its derivative)
    "N16-L2-sm-no-weights": dict(N=16, L=2, K=2, f=0, weights=None),
    "N17-L3-re-K3-weights-shape-nonuniform": dict(N=17, L=3, K=3, f=2, weights=True, shape=True, nonuniform=True),
    "N32-L2-ss-pertraj": dict(N=32, L=2, K=2, f=1, per_traj=True),
    "N32-L1-sm": dict(N=32, L=1, K=2, f=0),
    "N33-L2-sm-general-skewed": dict(N=33, L=2, K=2, f=0, herm=False, skew=3),
    "N40-L2-re": dict(N=40, L=2, K=1, f=2),
    "N48-L1-ss-K1-long-interval": dict(N=48, L=1, K=1, f=1, dt=4.0),
    "N49-L2-re": dict(N=49, L=2, K=2, f=2, nv=1),
    "N64-L2-sm-herm": dict(N=64, L=2, K=2, f=0, nv=1),
    "N64-L7-ss-general": dict(N=64, L=7, K=1, f=1, herm=False, amp=1.0, nv=1),
    # L = 8 with more than one wave: 2 + 2 L = 18 chains take two 16-column tiles (hvp_backward_kernel<NP, 2>), NW = NP / 16
    "N17-L8-sm-K2-shape": dict(N=17, L=8, K=2, f=0, amp=1.0, shape=True, weights=True, nonuniform=True, nv=1),   # NP 32, padded
    "N48-L8-ss-general": dict(N=48, L=8, K=1, f=1, amp=1.0, herm=False, nv=1),                                   # NP 48, full
    "N64-L8-re-pertraj": dict(N=64, L=8, K=2, f=2, amp=1.0, per_traj=True, nv=1),                                # NP 64
    # every interval is cut: all eighteen chains carry from one sub-step to the next across both tiles
    "N33-L8-ss-long": dict(N=33, L=8, K=1, f=1, amp=1.0, dt=4.0, nv=1),
}
LONG_INTERVALS = ("N48-L1-ss-K1-long-interval", "N33-L8-ss-long")
_cache = {}


def case(name):
    """(problem, directions, reference): computed once and shared.  Two directions; one where the reference is expensive
    (a 4N x 4N exponential per cell, control and direction)"""
    if name not in _cache:
        c = dict(CASES[name])
        f, nv = c.pop("f"), c.pop("nv", 2)
        pr = make_case(seed=1000 + sum(map(ord, name)), **c)
        V = hr.directions(sum(map(ord, name)), nv, pr["L"] * N_T)
        want = hr.evaluate(pr, pr["pulsevals"], V, f)
        _cache[name] = (pr, f, V, want)
    return _cache[name]


def assert_second_tile_agrees(got, want, L, label=""):
    """L = 8: the chains p'_6, p'_7 live in the second column tile of the backward kernel, and only the rows of H v that belong
    to the controls 6 and 7 depend on it.  Those rows by themselves, scaled by their own maximum -- which the reference alone must
    put at 1e-3 or more, so that the bound is relative there too.  Nothing to do below L = 8 (one tile)."""
    if L < 8:
        return None
    rows = lambda a: np.asarray(a, dtype=float).reshape(-1, L, N_T)[:, 6:8]   # noqa: E731 -- control-major [l * N_T + n]
    assert np.abs(rows(want)).max() >= 1e-3, float(np.abs(rows(want)).max())
    return hr.assert_hvp_agrees(rows(got), rows(want), label + " rows of the controls 6, 7")


@pytest.mark.parametrize("name", list(CASES))
def test_hvp_against_the_reference(name):
    pr, f, V, want = case(name)
    hr.assert_order_one(want)
    with handle(pr, f) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        Hv = h.hvp(V)
        info = h.hvp_info()
    assert abs(J - want["J"]) <= 1e-12 and np.abs(G - want["G"]).max() <= hr.tol_hv(want["G"])
    hr.assert_hvp_agrees(Hv, want["Hv"], name)
    assert (assert_second_tile_agrees(Hv, want["Hv"], pr["L"], name) is not None) == (pr["L"] == 8)
    print(info)
    steps = 2 * pr["K"] * len(V) * N_T
    if name in LONG_INTERVALS:
        # beta_n dt_n / theta: the norm estimate of the generator is ~ 1 (GUE scaled to spectral radius ~ 1) plus the control,
        # every interval is 4 long and theta = 3, so every interval is cut at least once
        assert info["series_steps"] >= 2 * steps, info
        assert info["series_steps"] % (2 * len(V)) == 0
    else:
        assert info["series_steps"] == steps, info
    assert info["series_terms"] > info["series_steps"] and info["bytes"] > 0 and info["ms"] > 0


def test_route_independence_at_n64():
    """after grape_eval without G, after the matrix-free propagator, after sequential sweeps and after grape_forward alone:
    each against the reference, and the four agree to rounding (the stored forward states differ in the last bits)"""
    pr, f, V, want = case("N64-L2-sm-herm")
    got = {}
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"], gradient=False)
        got["eval-no-G"] = h.hvp(V)
        h.set_fused_sweeps(False)
        h.eval(pr["pulsevals"])
        got["sequential-sweeps"] = h.hvp(V)
        h.forward(pr["pulsevals"])
        got["forward-alone"] = h.hvp(V)
    with handle(pr, f, prop_method=g.PROP_SERIES) as h:
        h.eval(pr["pulsevals"])
        got["series"] = h.hvp(V)
    for tag, Hv in got.items():
        hr.assert_hvp_agrees(Hv, want["Hv"], tag)
    # to rounding: the routes store forward states that differ in the last bits (1e-15 relative), H v is linear in them
    first = got["eval-no-G"]
    for tag, Hv in got.items():
        print(tag, float(np.abs(Hv - first).max() / np.abs(first).max()))
        assert np.abs(Hv - first).max() <= 1e-12 * np.abs(first).max(), tag
    pr, f, V, want = case("N49-L2-re")
    # N = 49 after the matrix-free propagator: the handle pads to 64 there (48 with the exponential)
    with handle(pr, f, prop_method=g.PROP_SERIES) as h:
        h.eval(pr["pulsevals"])
        hr.assert_hvp_agrees(h.hvp(V), want["Hv"], "N49-series")


@pytest.mark.parametrize("dirs", [None, 2])
def test_directions_do_not_see_each_other(monkeypatch, dirs):
    """nv = 5 in one call equals five calls, bit for bit -- also when the launch groups are forced to two directions"""
    if dirs:
        monkeypatch.setenv("GRAPE_HVP_DIRS", str(dirs))
    pr, f, _, _ = case("N17-L3-re-K3-weights-shape-nonuniform")
    V = hr.directions(77, 5, pr["L"] * N_T)
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        all5 = h.hvp(V)
        assert h.hvp_info()["dirs_per_group"] == (dirs or 5)
        again = h.hvp(V)
        single = np.stack([h.hvp(v) for v in V])
        pair = h.hvp(V[[3, 1]])
    assert np.array_equal(all5, again)
    assert np.array_equal(all5, single)
    assert np.array_equal(pair, all5[[3, 1]])


def test_symmetry_on_the_device():
    pr, f, V, _ = case("N33-L2-sm-general-skewed")
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        Hv = h.hvp(V)
    a, b = float(V[0] @ Hv[1]), float(V[1] @ Hv[0])
    print(dict(vHw=a, wHv=b))
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))


def test_two_tile_directions_do_not_see_each_other(monkeypatch):
    """L = 8 at NP = 32: three directions in one launch group and in three groups of one, bit for bit -- a direction does not
    depend on its launch group when its chains take two column tiles"""
    pr, f, _, _ = case("N17-L8-sm-K2-shape")
    V = hr.directions(79, 3, pr["L"] * N_T)
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        all3 = h.hvp(V)
        assert h.hvp_info()["dirs_per_group"] == 3
    monkeypatch.setenv("GRAPE_HVP_DIRS", "1")
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        one_by_one = h.hvp(V)
        assert h.hvp_info()["dirs_per_group"] == 1
    assert np.abs(all3.reshape(3, pr["L"], N_T)[:, 6:8]).max() >= 1e-3
    assert np.array_equal(all3, one_by_one)


def test_two_tile_symmetry_on_the_device():
    """v.(H w) = w.(H v) at L = 8, NP = 48: both sides mix rows of tile 0 with the rows of the controls 6 and 7 (tile 1)"""
    pr, f, _, _ = case("N48-L8-ss-general")
    V = hr.directions(78, 2, pr["L"] * N_T)
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        Hv = h.hvp(V)
    a, b = float(V[0] @ Hv[1]), float(V[1] @ Hv[0])
    tile1 = [float(V[i].reshape(pr["L"], N_T)[6:8].ravel() @ Hv[1 - i].reshape(pr["L"], N_T)[6:8].ravel()) for i in (0, 1)]
    print(dict(vHw=a, wHv=b, of_which_tile_1=tile1))
    assert abs(a - b) <= 1e-10 * max(abs(a), abs(b))


def test_no_side_effect_on_the_evaluation():
    pr, f, V, _ = case("N16-L2-re")
    for kw in (dict(), dict(prop_method=g.PROP_SERIES)):
        with handle(pr, f, **kw) as h:
            for _ in range(4):        # (beyond the second evaluation the captured graph replays)
                J0, G0, tau0 = h.eval(pr["pulsevals"])
            dJdt0 = h.time_gradient()
            h.hvp(V)
            assert np.array_equal(h.time_gradient(), dJdt0)
            for _ in range(3):
                J1, G1, tau1 = h.eval(pr["pulsevals"])
                assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(tau1, tau0)
                h.hvp(V[0])


def _refused(h, V, what):
    with pytest.raises(g.GrapeHipError) as ei:
        h.hvp(V)
    assert ei.value.code == -1, ei.value
    assert "grape_hvp" in str(ei.value) and what in str(ei.value), str(ei.value)


def test_refusals_leave_the_handle_usable():
    pr, f, V, _ = case("N16-L2-re")
    x = pr["pulsevals"]
    with handle(pr, f) as h:
        _refused(h, V, "no valid forward state")                        # nothing evaluated yet
        J0, G0, tau0 = h.eval(x)
        h.eval_batch(np.stack([x, 0.9 * x]))
        _refused(h, V, "grape_eval_batch")
        J1, G1, tau1 = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(tau1, tau0)
        h.hvp(V)
        h.set_tlist(pr["tlist"] * 1.25)
        _refused(h, V, "grape_set_tlist")
        h.set_tlist(pr["tlist"])
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
    # the built-in running cost
    D = np.diag(np.arange(16.0)).astype(complex)
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=f, D=D, lambda_b=0.1) as h:
        J0, G0, _ = h.eval(x)
        _refused(h, V, "running cost")
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
    # no targets
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], None, pr["weights"], functional=f) as h:
        h.forward(x)
        _refused(h, V, "no target states")
        h.forward(x)
    # a split-phase shard
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=f, K_total=4) as h:
        tau0 = h.forward(x)
        _refused(h, V, "shard")
        assert np.array_equal(h.forward(x), tau0)
    # N = 65
    big = synth.make_problem(65, 1, N_T, 1, seed=5)
    with g.GrapeHip(big["H0"], big["Hc"], big["tlist"], big["psi0"], big["target"], big["weights"]) as h:
        J0, G0, _ = h.eval(big["pulsevals"])
        _refused(h, np.ones(N_T), "N > 64")
        J1, G1, _ = h.eval(big["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)
    # an open-system handle
    op = synth.make_open_problem(4, 1, N_T, 1, 1, seed=5)
    with g.GrapeHipOpen(op["H0"], op["Hc"], op["cops"], op["tlist"], op["rho0"], op["target"]) as h:
        J0, G0, _ = h.eval(op["pulsevals"])
        _refused(h, np.ones(N_T), "open-system")
        J1, G1, _ = h.eval(op["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)


def test_trust_region_newton_reaches_the_lbfgs_threshold():
    """the TLS problem of tests/test_gpu_optimize.py with method="trust-ncg": the threshold that test uses for L-BFGS-B"""
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
    res = G.optimize([traj], tlist, J_T=G.J_T_sm, iter_stop=20, method="trust-ncg", rethrow_exceptions=True)
    print(res.J_T, res.message, res.iter)
    assert not res.message.startswith("Exception"), res.message
    assert res.J_T < 1e-3
