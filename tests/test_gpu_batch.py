"""grape_eval_batch on the GPU: many pulse vectors through one handle (include/grape_hip.h).

Bars.  Against the C oracle, one call per set, the bars tests/test_gpu_parity.py states for one evaluation:
    |dJ| <= 1e-12,   |dtau_k| <= 1e-12,   ||dG||_inf <= 1e-10 * max(||G||_inf, 1e-3).
Against ``h.eval`` of the same handle, set by set: TWICE those (triangle inequality: both sit within the bar of the oracle).
Where the text says "bit for bit" the comparison is ``np.array_equal``.
"""
import numpy as np
import pytest

import grape_jl_amd as g
from grape_jl_amd import synth

pytestmark = pytest.mark.gpu

TOL_J = 1e-12
TOL_TAU = 1e-12
SX = np.array([[0, 1], [1, 0]], dtype=complex)


def tol_G(Gref):
    return 1e-10 * max(np.abs(Gref).max(), 1e-3)


def _nonuniform(N_T, seed=5, lo=0.3, span=0.4):
    u = synth.uniform01(seed, N_T)
    return np.concatenate([[0.0], np.cumsum(lo + span * u)])


def _pulse_sets(pr, P, seed=91):
    """P different pulse vectors around the problem's own: [P, L*N_T]"""
    LN = pr["L"] * pr["N_T"]
    u = 2.0 * synth.uniform01(seed, P * LN).reshape(P, LN) - 1.0
    return pr["pulsevals"][None, :] + 0.15 * u


def _problem(N, L, K, N_T=12, seed=7, herm=True, per_traj=False, shape=False, weights=False, nonuniform=False):
    pr = synth.make_problem(N, L, N_T, K, seed=seed, hermitian=herm)
    kw = {}
    if per_traj:   # control operators per trajectory: [K, L, N, N]
        pr["Hc"] = np.stack([np.stack([synth.gue(synth.subseed(seed, 500 + 10 * k + l), N) for l in range(L)]) for k in range(K)])
    if not herm:   # general control operators as well
        z = synth.normal(synth.subseed(seed, 8), 2 * N * N)
        pr["Hc"] = pr["Hc"] + 0.1 * (z[0::2] + 1j * z[1::2]).reshape(N, N) / np.sqrt(N)
    if shape:
        kw["shape"] = 0.5 + synth.uniform01(synth.subseed(seed, 9), L * N_T).reshape(L, N_T)
    if weights:
        pr["weights"] = 0.5 + synth.uniform01(synth.subseed(seed, 10), K)
    if nonuniform:
        pr["tlist"] = _nonuniform(N_T, seed=seed)
    return pr, kw


def _handle(pr, functional=0, **kw):
    return g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=functional, **kw)


def _oracle(ref, pr, x, functional, kw, gradient=True):
    Hc, xx = pr["Hc"], x
    if "shape" in kw:   # the oracle has no shape argument: a_l = shape_ln eps_nl enters the generator, dJ/d eps = shape dJ/d a
        xx = x * kw["shape"].reshape(-1)
    J, G, tau = ref.evaluate(pr["H0"], Hc, pr["tlist"], xx, pr["psi0"], pr["target"], pr["weights"], functional=functional,
                             gradient=gradient)[:3]
    if gradient and "shape" in kw:
        G = G * kw["shape"].reshape(-1)
    return J, G, tau


# a covering set: every value of N in {2, 5, 16}, L in {1, 3}, K in {1, 4}, P in {1, 3, 17}, the three functionals, and each
# of shape / weights / non-uniform grid / general generators / control operators per trajectory, alone and combined
CASES = [
    dict(N=2, L=1, K=1, P=1, f=0),
    dict(N=2, L=3, K=4, P=3, f=1, shape=True),
    dict(N=2, L=1, K=4, P=17, f=2, weights=True, nonuniform=True),
    dict(N=5, L=1, K=1, P=3, f=1, nonuniform=True),
    dict(N=5, L=3, K=4, P=17, f=0, weights=True),
    dict(N=5, L=3, K=1, P=1, f=2, herm=False),
    dict(N=5, L=1, K=4, P=3, f=0, per_traj=True, shape=True),
    dict(N=16, L=1, K=1, P=17, f=0),
    dict(N=16, L=3, K=4, P=3, f=0, shape=True, weights=True, nonuniform=True),
    dict(N=16, L=1, K=4, P=1, f=1, herm=False),
    dict(N=16, L=3, K=4, P=17, f=2, per_traj=True),
    dict(N=16, L=3, K=1, P=3, f=1, herm=False, shape=True, nonuniform=True),
    dict(N=16, L=1, K=4, P=3, f=2, herm=False, per_traj=True, weights=True),
    dict(N=16, L=1, K=4, P=17, f=1, N_T=70),
]


def _case_id(c):
    return "-".join(f"{k}{v}" if not isinstance(v, bool) else k for k, v in c.items())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_parity_per_set(ref, monkeypatch, case):
    """every set of a batch against the oracle (the bars of one evaluation) and against h.eval of the same handle (twice those)"""
    monkeypatch.setenv("GRAPE_BATCH", "1")
    c = dict(case)
    P, f = c.pop("P"), c.pop("f")
    pr, kw = _problem(c.pop("N"), c.pop("L"), c.pop("K"), **c)
    X = _pulse_sets(pr, P)
    with _handle(pr, f, **kw) as h:
        J, G, tau = h.eval_batch(X)
        assert h.batch_info()["route"] == 1, h.batch_info()
        assert J.shape == (P,) and G.shape == X.shape and tau.shape == (P, pr["K"])
        for p in range(P):
            Jr, Gr, taur = _oracle(ref, pr, X[p], f, kw)
            print(f"set {p}: dJ {abs(J[p] - Jr):.2e} dtau {np.abs(tau[p] - taur).max():.2e} dG {np.abs(G[p] - Gr).max():.2e} (bar {tol_G(Gr):.2e})")
            assert abs(J[p] - Jr) <= TOL_J, (p, J[p], Jr)
            assert np.abs(tau[p] - taur).max() <= TOL_TAU, p
            assert np.abs(G[p] - Gr).max() <= tol_G(Gr), (p, np.abs(G[p] - Gr).max())
            J1, G1, tau1 = h.eval(X[p])
            assert abs(J[p] - J1) <= 2 * TOL_J and np.abs(tau[p] - tau1).max() <= 2 * TOL_TAU
            assert np.abs(G[p] - G1).max() <= 2 * tol_G(Gr)


def test_two_level_closed_forms(ref, monkeypatch):
    """eight amplitudes at once.  H = eps sigma_x, |0> -> |1>, J_T_sm (tests/test_gpu_time_grid.py): J = 1 - sin^2(eps T) and
    dJ/d eps_n = -dt sin(2 eps T).  The README problem H = sigma_z + eps sigma_x: Rabi's formula, J = 1 - (eps / W)^2 sin^2(W T)
    with W = sqrt(1 + eps^2); its gradient against the oracle."""
    monkeypatch.setenv("GRAPE_BATCH", "1")
    amps = np.array([0.05, 0.1, 0.2, 0.3, 0.45, 0.6, 0.8, 1.1])
    T, N_T = 2.0, 20
    tl = np.linspace(0.0, T, N_T + 1)
    X = np.repeat(amps[:, None], N_T, axis=1)
    with g.GrapeHip(np.zeros((1, 2, 2), complex), SX[None], tl, np.array([[1, 0]], complex), np.array([[0, 1]], complex)) as h:
        J, G, tau = h.eval_batch(X)
        assert h.batch_info()["route"] == 1
    assert np.abs(J - (1.0 - np.sin(amps * T) ** 2)).max() <= TOL_J
    Gw = -(T / N_T) * np.sin(2 * amps * T)
    assert np.abs(G - Gw[:, None]).max() <= tol_G(Gw)
    pr = synth.readme_tls()
    X = np.repeat(amps[:, None], pr["N_T"], axis=1)
    with _handle(pr) as h:
        J, G, tau = h.eval_batch(X)
        assert h.batch_info()["route"] == 1
    W = np.sqrt(1.0 + amps ** 2)
    assert np.abs(J - (1.0 - (amps / W) ** 2 * np.sin(W * 5.0) ** 2)).max() <= TOL_J
    for p in range(len(amps)):
        Jr, Gr, taur = _oracle(ref, pr, X[p], 0, {})
        assert abs(J[p] - Jr) <= TOL_J and np.abs(tau[p] - taur).max() <= TOL_TAU
        assert np.abs(G[p] - Gr).max() <= tol_G(Gr)


def test_a_set_does_not_see_its_neighbours(monkeypatch):
    """the same pulse vector alone, at p = 5 of 8 among random others, and in a run cut into launch groups of two: bit for bit"""
    monkeypatch.setenv("GRAPE_BATCH", "1")
    pr, kw = _problem(16, 3, 4, N_T=40, shape=True, weights=True)
    X = _pulse_sets(pr, 8, seed=17)
    x = X[5].copy()
    with _handle(pr, 0, **kw) as h:
        J1, G1, tau1 = h.eval_batch(x[None])
        assert h.batch_info() == dict(route=1, sets_per_group=1, groups=1, bytes=h.batch_info()["bytes"])
        J8, G8, tau8 = h.eval_batch(X)
        info = h.batch_info()
        assert info["route"] == 1 and info["sets_per_group"] == 8 and info["groups"] == 1 and info["bytes"] > 0
        again = h.eval_batch(X)
    assert J1[0] == J8[5] and np.array_equal(G1[0], G8[5]) and np.array_equal(tau1[0], tau8[5])
    assert np.array_equal(again[0], J8) and np.array_equal(again[1], G8) and np.array_equal(again[2], tau8)
    monkeypatch.setenv("GRAPE_BATCH_SETS", "2")
    with _handle(pr, 0, **kw) as h:
        Jg, Gg, taug = h.eval_batch(X[:7])   # (three full groups and a single set)
        info = h.batch_info()
        assert info["route"] == 1 and info["sets_per_group"] == 2 and info["groups"] == 4
    assert np.array_equal(Jg, J8[:7]) and np.array_equal(Gg, G8[:7]) and np.array_equal(taug, tau8[:7])


def _dpen(N, seed=77):
    A = synth.gue(seed, N)
    return A @ A.conj().T


LOOP_CASES = {
    "N24": (dict(N=24), {}),
    "taylor": (dict(N=8), dict(gradient_method=g.GRAD_TAYLOR)),
    "series": (dict(N=8), dict(prop_method=g.PROP_SERIES)),
    "dpen": (dict(N=8), dict(D=_dpen(8), lambda_b=0.3)),
    "two_shards_one_device": (dict(N=8), dict(devices=[0, 0])),
}


@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_the_loop_route(monkeypatch, name):
    """outside the envelope of the batched kernels: one ordinary evaluation per set, bit for bit P h.eval calls (made BEFORE the
    batch call on the same handle; from the third on they replay the captured graph), even with GRAPE_BATCH=1"""
    monkeypatch.setenv("GRAPE_BATCH", "1")
    shape, kw = LOOP_CASES[name]
    pr, _ = _problem(shape["N"], 2, 4, N_T=10, seed=23)
    X = _pulse_sets(pr, 3)
    with _handle(pr, 0, **kw) as h:
        one = [h.eval(X[p]) for p in range(3)]
        J, G, tau = h.eval_batch(X)
        assert h.batch_info()["route"] == 0 and h.batch_info()["groups"] == 3
        for p in range(3):
            assert J[p] == one[p][0] and np.array_equal(G[p], one[p][1]) and np.array_equal(tau[p], one[p][2])


def test_functional_only(monkeypatch):
    monkeypatch.setenv("GRAPE_BATCH", "1")
    pr, kw = _problem(16, 1, 4, N_T=30, weights=True)
    X = _pulse_sets(pr, 5)
    for f in (0, 1, 2):
        with _handle(pr, f, **kw) as h:
            J, G, tau = h.eval_batch(X)
            J0, G0, tau0 = h.eval_batch(X, gradient=False)
            assert G0 is None and h.batch_info()["route"] == 1
        assert np.abs(J0 - J).max() <= TOL_J and np.abs(tau0 - tau).max() <= TOL_TAU


def test_errors(monkeypatch):
    monkeypatch.setenv("GRAPE_BATCH", "1")
    pr, kw = _problem(5, 1, 2, N_T=6)
    LN = pr["L"] * pr["N_T"]
    X = _pulse_sets(pr, 3)
    with _handle(pr) as h:
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval_batch(np.empty((0, LN)))
        assert ei.value.code == -1
        J = np.zeros(3)
        with pytest.raises(g.GrapeHipError) as ei:   # NULL J
            h._chk(h._lib.grape_eval_batch(h._h, 3, X.ctypes.data, None, None, None))
        assert ei.value.code == -1
        with pytest.raises(g.GrapeHipError) as ei:   # NULL pulsevals
            h._chk(h._lib.grape_eval_batch(h._h, 3, None, J.ctypes.data, None, None))
        assert ei.value.code == -1
        Jb, Gb, _ = h.eval_batch(X)                  # the handle is unchanged and usable
        assert h.batch_info()["route"] == 1 and np.isfinite(Jb).all() and np.isfinite(Gb).all()
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], K_total=4) as h:   # a split-phase shard
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval_batch(X)
        assert ei.value.code == -1
        h.forward(X[0])
    # exactly one set trips the chi-norm guard (optimize.jl:1021-1025): H = eps sigma_x, |0> -> |1>, J_T_sm -- the set with eps = 0 on
    # every interval has U = 1 and tau = 0 exactly, the sets with eps = 0.3 are fine
    N_T = 4
    tl = np.linspace(0.0, 1.0, N_T + 1)
    Xe = np.full((4, N_T), 0.3)
    Xe[2] = 0.0
    with g.GrapeHip(np.zeros((1, 2, 2), complex), SX[None], tl, np.array([[1, 0]], complex), np.array([[0, 1]], complex)) as h:
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval_batch(Xe)
        assert ei.value.code == -3 and "pulse set 2" in str(ei.value) and "chi" in str(ei.value)
        J, G, tau = h.eval_batch(Xe[[0, 1, 3]])
        assert h.batch_info()["route"] == 1
        assert np.abs(J - (1.0 - np.sin(0.3) ** 2)).max() <= TOL_J
        J0, _, tau0 = h.eval_batch(Xe, gradient=False)   # the functional alone is fine for every set
        assert abs(J0[2] - 1.0) <= 1e-15 and tau0[2, 0] == 0.0


def test_state_after_a_batch_call(monkeypatch):
    monkeypatch.setenv("GRAPE_BATCH", "1")
    pr, kw = _problem(16, 1, 4, N_T=80, seed=31)
    X = _pulse_sets(pr, 6)
    x = pr["pulsevals"]
    with _handle(pr) as h:
        before = [h.eval(x) for _ in range(4)]       # (the third and fourth replay the captured graph)
        h.time_gradient()
        h.eval_batch(X)
        assert h.batch_info()["route"] == 1
        with pytest.raises(g.GrapeHipError) as ei:
            h.time_gradient()
        assert ei.value.code == -1
        after = h.eval(x)
        for b in before:
            assert b[0] == after[0] and np.array_equal(b[1], after[1]) and np.array_equal(b[2], after[2])
        h.time_gradient()                            # ... and an ordinary evaluation with a gradient brings it back
        # a new grid: the batch route reads it, bit for bit like a fresh handle on that grid
        tl2 = _nonuniform(pr["N_T"], seed=3)
        h.set_tlist(tl2)
        got = h.eval_batch(X)
    pr2 = dict(pr, tlist=tl2)
    with _handle(pr2) as h2:
        want = h2.eval_batch(X)
        assert h2.batch_info()["route"] == 1
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_route_rule_and_forced_loop(monkeypatch):
    """GRAPE_BATCH=0 forces the loop inside the envelope; without the variable a single set takes the ordinary path"""
    pr, kw = _problem(16, 1, 2, N_T=20)
    X = _pulse_sets(pr, 4)
    monkeypatch.setenv("GRAPE_BATCH", "0")
    with _handle(pr) as h:
        J0, G0, tau0 = h.eval_batch(X)
        assert h.batch_info()["route"] == 0
    monkeypatch.delenv("GRAPE_BATCH")
    with _handle(pr) as h:
        h.eval_batch(X[:1])
        assert h.batch_info()["route"] == 0
        J1, G1, tau1 = h.eval_batch(X)
        assert h.batch_info()["route"] == 1
    assert np.abs(J1 - J0).max() <= 2 * TOL_J and np.abs(tau1 - tau0).max() <= 2 * TOL_TAU
    assert np.abs(G1 - G0).max() <= 2 * tol_G(G0)
