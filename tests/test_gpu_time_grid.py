"""dJ/d(dt_n) (grape_get_time_gradient) and grape_set_tlist on the MI355X (ABI v7).

The reference value is the pseudo-control identity dt_n dJ/d(dt_n) = G^c_n + sum_l eps_nl G_nl of the oracle's gradient
(tests/test_time_grid_host.py checks it against central differences of the oracle's J)."""
import numpy as np
import pytest

import grape_jl_amd as g
from grape_jl_amd import synth
from test_time_grid_host import (LONG_CASES, LONG_IDS, assert_every_block_has_signal, central_dJdt, intervals_per_workgroup,
                                 long_case, padded_size, pseudo_control_dJdt, running_cost_weight_term)

pytestmark = pytest.mark.gpu

TOL = 1e-10
SX = np.array([[0, 1], [1, 0]], dtype=complex)


def _nonuniform(N_T, seed=5, lo=0.3, span=0.4):
    u = synth.uniform01(seed, N_T)
    return np.concatenate([[0.0], np.cumsum(lo + span * u)])


def _close(got, ref, tol=TOL):
    scale = max(np.abs(ref).max(), 1e-3)
    assert np.abs(got - ref).max() <= tol * scale, (np.abs(got - ref).max(), scale)


def _tls(eps, T, N_T, **kw):
    tl = np.linspace(0.0, T, N_T + 1)
    return g.GrapeHip(np.zeros((1, 2, 2), complex), SX[None], tl, np.array([[1, 0]], complex),
                      np.array([[0, 1]], complex), **kw), np.full(N_T, eps)


def test_closed_form_two_level():
    """H = eps sigma_x, |0> -> |1>, J_T_sm: J = 1 - sin^2(eps T), so every dJ/d(dt_n) = -eps sin(2 eps T)."""
    eps, T, N_T = 0.3, 2.0, 20
    h, x = _tls(eps, T, N_T)
    with h:
        for _ in range(3):   # (the third evaluation replays the captured graph)
            h.eval(x)
            d = h.time_gradient()
            assert np.abs(d + eps * np.sin(2 * eps * T)).max() <= 1e-13, d


def test_duration_minimisation_lands_on_the_speed_limit():
    """A 1-D minimisation of T with set_tlist + time_gradient (dJ/dT = sum_n dt_n / T dJ/d(dt_n)) finds T* = pi / (2 eps)."""
    eps, N_T = 0.3, 16
    h, x = _tls(eps, 3.0, N_T)

    def dJdT(T):
        tl = np.linspace(0.0, T, N_T + 1)
        h.set_tlist(tl)
        h.eval(x)
        return float(np.sum(np.diff(tl) / T * h.time_gradient()))

    with h:
        a, b = 3.0, 4.0
        fa, fb = dJdT(a), dJdT(b)
        for _ in range(40):   # secant steps on dJ/dT = 0
            if abs(fb) < 1e-15:
                break
            a, b, fa = b, b - fb * (b - a) / (fb - fa), fb
            fb = dJdT(b)
        assert abs(b - np.pi / (2 * eps)) <= 1e-8, b


CASES = [
    # id, N, L, K, N_T, functional, gradient_method, prop, fused, herm, per-trajectory controls, env
    ("n2", 2, 1, 3, 12, 0, g.GRAD_GRADGEN, g.PROP_EXP, True, True, False, {}),
    ("n16-scan", 16, 2, 4, 40, 1, g.GRAD_TAYLOR, g.PROP_EXP, True, True, True, {"GRAPE_SCAN16": "1"}),
    ("n16-seq", 16, 3, 3, 24, 2, g.GRAD_GRADGEN, g.PROP_EXP, False, True, False, {"GRAPE_SCAN16": "0"}),
    ("n40-general", 40, 3, 3, 10, 2, g.GRAD_GRADGEN, g.PROP_EXP, False, False, False, {}),
    ("n64-asm", 64, 2, 3, 20, 0, g.GRAD_GRADGEN, g.PROP_EXP, True, True, False, {}),
    ("n64-general-taylor", 64, 1, 2, 12, 1, g.GRAD_TAYLOR, g.PROP_EXP, True, False, True, {}),
    ("n64-series", 64, 3, 2, 8, 1, g.GRAD_GRADGEN, g.PROP_SERIES, True, True, False, {}),
    ("n100-blocked", 100, 1, 2, 6, 0, g.GRAD_TAYLOR, g.PROP_EXP, True, True, False, {}),
    ("n100-series-general", 100, 2, 2, 5, 2, g.GRAD_GRADGEN, g.PROP_SERIES, True, False, False, {}),
    ("n256-blocked", 256, 1, 1, 3, 0, g.GRAD_GRADGEN, g.PROP_EXP, True, True, False, {}),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_the_oracle(ref, monkeypatch, case):
    cid, N, L, K, N_T, fn, gm, pm, fused, herm, per_traj, env = case
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    pr = synth.make_problem(N, L, N_T, K, seed=31 + N, hermitian=herm)
    Hc = np.stack([pr["Hc"] * (1.0 + 0.1 * k) for k in range(K)]) if per_traj else pr["Hc"]
    tl = _nonuniform(N_T, seed=N)
    w = np.linspace(0.5, 1.5, K)
    with g.GrapeHip(pr["H0"], Hc, tl, pr["psi0"], pr["target"], w, functional=fn, gradient_method=gm,
                    prop_method=pm) as h:
        h.set_fused_sweeps(fused)
        _, G, _ = h.eval(pr["pulsevals"])
        d = h.time_gradient()
        wk = h.work()
    want = pseudo_control_dJdt(ref, pr["H0"], Hc, tl, pr["pulsevals"], pr["psi0"], pr["target"], weights=w,
                               functional=fn, gradient_method=gm)
    _close(d, want)
    if cid == "n64-asm":
        assert wk["asm_kernel"] == 1 and wk["walk_steps"] > 0, wk
    if cid == "n16-scan":
        assert wk["scan_block"] > 0, wk


# ---- beyond the first workgroup of time_grad_kernel -------------------------------------------------------------------------
# A workgroup owns CW = intervals_per_workgroup(NP) intervals (64 / 32 / 16); every case above stays inside one.  LONG_CASES
# (tests/test_time_grid_host.py, where the table is checked without a GPU) reaches n0 = blockIdx.x * CW > 0, the guarded tail of
# the last block, the g_b read across a block boundary and the reduction over more than four groups of 16 intervals.

def _report(label, got, ref_, tol=TOL):
    """deviation / tolerance of ``_close``, printed before it asserts"""
    scale = max(np.abs(ref_).max(), 1e-3)
    print(label, dict(ratio=float(np.abs(got - ref_).max() / (tol * scale)), scale=float(scale)))
    _close(got, ref_, tol)


def _long_handle(ref, cid, **kw):
    _, N, L, K, N_T, fn, herm, blocks = LONG_CASES[LONG_IDS.index(cid)]
    pr, tl, w, want = long_case(ref, cid)
    CW = intervals_per_workgroup(padded_size(N))
    assert -(-N_T // CW) == blocks, (N_T, CW)
    assert_every_block_has_signal(want, CW, cid)
    return g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], w, functional=fn, **kw), pr, want


@pytest.mark.parametrize("cid", LONG_IDS)
def test_long_grids_against_the_oracle(ref, cid):
    h, pr, want = _long_handle(ref, cid)
    with h:
        h.eval(pr["pulsevals"])
        d = h.time_gradient()
        wk = h.work()
    _report(cid, d, want)
    if cid.startswith("n64-"):
        assert wk["asm_kernel"] == 1, wk   # the headline route


@pytest.mark.parametrize("fused", [True, False], ids=["as-created-z", "sequential-rho"])
@pytest.mark.parametrize("cid", ["n16-one-column-over", "n64-three-blocks"])
def test_long_grids_in_both_backward_layouts(ref, cid, fused):
    """The two arms of the kernel's epilogue: after the concurrent sweeps the backward storage holds the unit states and the
    factor is z_k; after sequential sweeps it holds the true ones and the factor is rho_k."""
    h, pr, want = _long_handle(ref, cid)
    with h:
        if not fused:
            assert h.set_fused_sweeps(False) is False
        h.eval(pr["pulsevals"])
        d = h.time_gradient()
        wk = h.work()
        # (what the handle reports as active is what grape_eval ran: a handle as created has the switch on)
        assert h.set_fused_sweeps(fused) is fused
    print(cid, dict(fused=fused, scan_block=wk["scan_block"]))
    _report(f"{cid} fused={fused}", d, want)
    # 64 time steps and more, few trajectories: both layouts are written by the scanned sweeps
    assert wk["scan_block"] > 0, wk


def test_long_grid_running_cost_across_a_block_boundary(ref):
    """g_b(t_n) + g_b(t_{n+1}) at n = 63 reads the last point of block 0 and the first of block 1; n = 64 is block 1 alone"""
    N, L, K, N_T, lam = 16, 2, 2, 65, 0.3
    pr = synth.make_problem(N, L, N_T, K, seed=9)
    tl = _nonuniform(N_T, seed=11)
    D = _dpen(N)
    args = (pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], pr["target"])
    weight = running_cost_weight_term(ref, pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], D, lam)
    want = pseudo_control_dJdt(ref, *args, D=D, lambda_b=lam) + weight
    print(dict(weight_63=float(weight[63]), weight_64=float(weight[64])))
    assert abs(weight[63]) >= 1e-3 and abs(weight[64]) >= 1e-3
    assert_every_block_has_signal(want, intervals_per_workgroup(padded_size(N)), "running cost")
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], D=D, lambda_b=lam) as h:
        h.eval(pr["pulsevals"])
        d = h.time_gradient()
    _report("running cost, N_T = 65", d, want)


def test_long_grid_with_shape_and_per_trajectory_controls(ref):
    """n16-one-column-over with a shape and H_l per trajectory against the library's own pseudo-control route (the identity of
    test_shapes_against_the_pseudo_control_route_and_differences, without its differences)"""
    cid = "n16-one-column-over"
    _, N, L, K, N_T, fn, _, _ = LONG_CASES[LONG_IDS.index(cid)]
    pr, tl, w, _ = long_case(ref, cid)
    Hc = np.stack([pr["Hc"] * (1.0 + 0.1 * k) for k in range(K)])
    shape = 0.5 + synth.uniform01(23, L * N_T).reshape(L, N_T)
    x = pr["pulsevals"]
    with g.GrapeHip(pr["H0"], Hc, tl, pr["psi0"], pr["target"], w, functional=fn, shape=shape) as h:
        h.eval(x)
        d = h.time_gradient()
    Hp = np.concatenate([pr["H0"][:, None], Hc], axis=1)
    sp = np.concatenate([np.ones((1, N_T)), shape])
    with g.GrapeHip(np.zeros_like(pr["H0"]), Hp, tl, pr["psi0"], pr["target"], w, functional=fn, shape=sp) as hp:
        _, Gp, _ = hp.eval(np.concatenate([np.ones(N_T), x]))
    Gp = Gp.reshape(L + 1, N_T)
    want = (Gp[0] + np.sum(x.reshape(L, N_T) * Gp[1:], axis=0)) / np.diff(tl)
    assert_every_block_has_signal(want, intervals_per_workgroup(padded_size(N)), "shape, per-trajectory controls")
    _report("shape, per-trajectory controls, N_T = 65", d, want)


def test_long_grid_sharding():
    """n16-one-column-over with K = 4: two device shards behind one handle, and a 1 + 3 split-phase pair"""
    cid = "n16-one-column-over"
    _, N, L, _, N_T, fn, _, _ = LONG_CASES[LONG_IDS.index(cid)]
    K = 4
    pr = synth.make_problem(N, L, N_T, K, seed=31 + N)
    tl = _nonuniform(N_T, seed=N)
    w = np.linspace(0.5, 1.5, K)
    x = pr["pulsevals"]
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], w, functional=fn) as h:
        h.eval(x)
        d1 = h.time_gradient()
    assert np.abs(d1[:64]).max() >= 1e-3 and abs(d1[64]) >= 1e-3, d1
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], w, functional=fn, devices=[0, 0]) as h:
        h.eval(x)
        d2 = h.time_gradient()
    _report("devices=[0, 0]", d2, d1, tol=1e-14)
    parts, taus = [], []
    for lo, hi in ((0, 1), (1, 4)):
        sl = slice(lo, hi)
        hs = g.GrapeHip(pr["H0"][sl], pr["Hc"], tl, pr["psi0"][sl], pr["target"][sl], w[sl], functional=fn, K_total=K)
        taus.append((hs, hs.forward(x), hs.sums()))
    f = sum(complex(s[0], s[1]) for _, _, s in taus)
    for hs, _, _ in taus:
        hs.backward(f)
        parts.append(hs.time_gradient())
        hs.close()
    _report("1 + 3 split-phase", parts[0] + parts[1], d1, tol=1e-14)


@pytest.mark.parametrize("cid", ["n16-one-column-over", "n64-three-blocks"])
def test_long_grid_replay_gives_the_same_bits(ref, cid):
    h, pr, want = _long_handle(ref, cid)
    with h:
        got = []
        for _ in range(3):   # (N <= 64: the third evaluation replays the captured graph)
            h.eval(pr["pulsevals"])
            got.append(h.time_gradient())
    _report(cid + ", first evaluation", got[0], want)
    assert np.array_equal(got[2], got[0])


def test_gate_problem_with_generator_classes(ref):
    """K trajectories over KC = 1 generator class (one drift, the logical basis as initial states)."""
    N, L, N_T, K = 16, 2, 30, 4
    pr = synth.make_problem(N, L, N_T, K, seed=4)
    H0 = np.broadcast_to(pr["H0"][0], (K, N, N)).copy()
    psi0, target = np.eye(N, dtype=complex)[:K], np.eye(N, dtype=complex)[1:K + 1]
    tl = _nonuniform(N_T, seed=2)
    for fn in (0, 1):
        with g.GrapeHip(H0, pr["Hc"], tl, psi0, target, functional=fn) as h:
            h.eval(pr["pulsevals"])
            d = h.time_gradient()
        _close(d, pseudo_control_dJdt(ref, H0, pr["Hc"], tl, pr["pulsevals"], psi0, target, functional=fn))


def _dpen(N, seed=77):
    X = synth.normal(seed, 2 * N * N).reshape(2, N, N)
    D = (X[0] + 1j * X[1]) / 4
    return D + D.conj().T


@pytest.mark.parametrize("N", [16, 64])
def test_running_cost_adds_the_weight_term(ref, N):
    N_T, K, L, lam = 12, 2, 2, 0.3
    pr = synth.make_problem(N, L, N_T, K, seed=9)
    tl = _nonuniform(N_T, seed=11)
    D = _dpen(N)
    args = (pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], pr["target"])
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], D=D, lambda_b=lam) as h:
        h.eval(pr["pulsevals"])
        d = h.time_gradient()
    want = pseudo_control_dJdt(ref, *args, D=D, lambda_b=lam) + \
        running_cost_weight_term(ref, pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], D, lam)
    _close(d, want)


def test_shapes_against_the_pseudo_control_route_and_differences():
    """With a shape (which the oracle cannot take): the library's own pseudo-control route, and central differences of
    the library's J in dt_n (the shape values stay fixed per interval)."""
    N, L, N_T, K = 16, 2, 10, 2
    pr = synth.make_problem(N, L, N_T, K, seed=17)
    tl = _nonuniform(N_T, seed=7)
    shape = 0.5 + synth.uniform01(23, L * N_T).reshape(L, N_T)
    x = pr["pulsevals"]
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], shape=shape) as h:
        J0, _, _ = h.eval(x)
        d = h.time_gradient()
        fd = np.empty(N_T)
        for n in range(N_T):
            hh = 1e-5 * (tl[n + 1] - tl[n])
            Jpm = []
            for sgn in (1, -1):
                t2 = tl.copy()
                t2[n + 1:] += sgn * hh
                h.set_tlist(t2)
                Jpm.append(h.eval(x, gradient=False)[0])
            fd[n] = (Jpm[0] - Jpm[1]) / (2 * hh)
    Hp = np.concatenate([pr["H0"][:, None], np.broadcast_to(pr["Hc"], (K,) + pr["Hc"].shape)], axis=1)
    sp = np.concatenate([np.ones((1, N_T)), shape])
    with g.GrapeHip(np.zeros_like(pr["H0"]), Hp, tl, pr["psi0"], pr["target"], shape=sp) as hp:
        _, Gp, _ = hp.eval(np.concatenate([np.ones(N_T), x]))
    Gp = Gp.reshape(L + 1, N_T)
    # (G_nl = dJ/d eps_nl = shape_ln dJ/d a_ln: the identity sum_a a_a dJ/d a_a needs eps, not a = shape eps)
    want = (Gp[0] + np.sum(x.reshape(L, N_T) * Gp[1:], axis=0)) / np.diff(tl)
    _close(d, want)
    _close(d, fd, tol=1e-7)


def test_caller_chi_and_caller_running_cost(ref):
    N, L, N_T, K, lam = 16, 1, 10, 3, 0.4
    pr = synth.make_problem(N, L, N_T, K, seed=19)
    tl = _nonuniform(N_T, seed=13)
    D = _dpen(N, seed=5)
    args = (pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], pr["target"])
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], functional=g.J_T_RE) as h:
        h.set_fused_sweeps(False)
        h.eval(pr["pulsevals"])
        d_builtin = h.time_gradient()
        # J_T_re through the caller's chi: chi_k = target_k / (2K)
        h.forward(pr["pulsevals"])
        h.backward_chi(pr["target"] / (2 * K))
        _close(h.time_gradient(), d_builtin, tol=1e-13)
        # an arbitrary running cost handed over as data: xi = -D Psi; the library returns the propagation part
        h.forward(pr["pulsevals"])
        fw = h.storage(0)
        xi = -np.einsum("ij,knj->kni", D, fw)
        h.backward_xi(xi, lam)
        d_xi = h.time_gradient()
    gb = np.real(np.einsum("kni,ij,knj->kn", fw.conj(), D, fw))
    d_xi = d_xi + 0.5 * lam * np.sum(gb[:, :-1] + gb[:, 1:], axis=0)
    fd = central_dJdt(ref, *args, functional=g.J_T_RE, D=D, lambda_b=lam)
    _close(d_xi, fd, tol=1e-7)
    want = pseudo_control_dJdt(ref, *args, functional=g.J_T_RE, D=D, lambda_b=lam) + \
        running_cost_weight_term(ref, pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], D, lam)
    _close(d_xi, want)


def test_sharding():
    N, L, N_T, K = 16, 2, 20, 4
    pr = synth.make_problem(N, L, N_T, K, seed=3)
    tl = _nonuniform(N_T, seed=1)
    args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"])
    with g.GrapeHip(*args) as h:
        h.eval(pr["pulsevals"])
        d1 = h.time_gradient()
    with g.GrapeHip(*args, devices=[0, 0]) as h:
        h.eval(pr["pulsevals"])
        d2 = h.time_gradient()
    _close(d2, d1, tol=1e-14)
    parts, taus = [], []
    for lo, hi in ((0, 1), (1, 4)):
        sl = slice(lo, hi)
        hs = g.GrapeHip(pr["H0"][sl], pr["Hc"], tl, pr["psi0"][sl], pr["target"][sl], K_total=K)
        taus.append((hs, hs.forward(pr["pulsevals"]), hs.sums()))
    f = sum(complex(s[0], s[1]) for _, _, s in taus)
    for hs, _, _ in taus:
        hs.backward(f)
        parts.append(hs.time_gradient())
        hs.close()
    _close(parts[0] + parts[1], d1, tol=1e-14)


SET_CASES = [
    ("n16-graph", 16, 2, 3, 40, g.PROP_EXP, False, {}),
    ("n64-asm", 64, 2, 3, 20, g.PROP_EXP, False, {}),
    ("n100-blocked", 100, 1, 2, 6, g.PROP_EXP, False, {}),
    ("n32-series", 32, 2, 2, 10, g.PROP_SERIES, False, {}),
    ("n16-dpen", 16, 2, 2, 12, g.PROP_EXP, True, {}),
]


@pytest.mark.parametrize("case", SET_CASES, ids=[c[0] for c in SET_CASES])
def test_set_tlist_equals_a_fresh_handle(case):
    cid, N, L, K, N_T, pm, dpen, env = case
    pr = synth.make_problem(N, L, N_T, K, seed=41)
    t1 = _nonuniform(N_T, seed=3)
    # the second grid: steps up to 4x larger (more squarings on the blocked path)
    t2 = _nonuniform(N_T, seed=8, lo=0.5, span=3.5)
    kw = dict(prop_method=pm)
    if dpen:
        kw.update(D=_dpen(N), lambda_b=0.2)
    x = pr["pulsevals"]
    with g.GrapeHip(pr["H0"], pr["Hc"], t1, pr["psi0"], pr["target"], **kw) as h:
        for _ in range(3):   # N <= 64: the third evaluation is a captured graph
            h.eval(x)
        h.time_gradient()
        h.set_tlist(t2)
        with pytest.raises(g.GrapeHipError):
            h.time_gradient()   # (the states belong to the old grid)
        res = []
        for _ in range(3):
            J, G, tau = h.eval(x)
            res.append((J, G, tau, h.time_gradient()))
    with g.GrapeHip(pr["H0"], pr["Hc"], t2, pr["psi0"], pr["target"], **kw) as hf:
        for i in range(3):
            J, G, tau = hf.eval(x)
            d = hf.time_gradient()
            assert J == res[i][0]
            assert np.array_equal(G, res[i][1]) and np.array_equal(tau, res[i][2]) and np.array_equal(d, res[i][3])


def test_bad_grids_are_refused_and_change_nothing():
    N, L, N_T, K = 16, 1, 8, 2
    pr = synth.make_problem(N, L, N_T, K, seed=2)
    tl = _nonuniform(N_T)
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"]) as h:
        J0, G0, _ = h.eval(pr["pulsevals"])
        d0 = h.time_gradient()
        for bad in (np.r_[tl[:4], tl[3], tl[5:]], np.r_[tl[:3], np.nan, tl[4:]], np.r_[tl[:-1], np.inf]):
            with pytest.raises(g.GrapeHipError) as e:
                h.set_tlist(bad)
            assert e.value.code == -1
            assert np.array_equal(h.time_gradient(), d0)   # (a refused grid leaves the last results in place)
        J1, G1, _ = h.eval(pr["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(h.time_gradient(), d0)


def test_no_interference_and_errors():
    N, L, N_T, K = 64, 2, 16, 3
    pr = synth.make_problem(N, L, N_T, K, seed=6)
    tl = _nonuniform(N_T)
    args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"])
    x = pr["pulsevals"]
    with g.GrapeHip(*args) as a, g.GrapeHip(*args) as b:
        with pytest.raises(g.GrapeHipError) as e:
            a.time_gradient()   # before any evaluation
        assert e.value.code == -1
        for _ in range(5):
            ra = a.eval(x)
            rb = b.eval(x)
            b.time_gradient()
            assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        a.eval(x, gradient=False)
        with pytest.raises(g.GrapeHipError) as e:
            a.time_gradient()   # the last evaluation had no gradient
        assert e.value.code == -1
        a.forward(x)
        with pytest.raises(g.GrapeHipError) as e:
            a.time_gradient()   # between forward and backward
        assert e.value.code == -1
        sm = a.sums()
        a.backward(complex(sm[0], sm[1]))
        d = a.time_gradient()
        assert np.array_equal(d, b.time_gradient())
