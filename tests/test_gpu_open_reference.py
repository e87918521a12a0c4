"""Open-system kernels (grape_create_open) against the plain matrix-form reference of tests/open_reference.py, beyond the
reach of the C oracle: 16 < d <= 64 (the NP = 32 / 48 / 64 instantiations), up to J = 8 collapse operators, L from 1 to 5 --
needs an MI355X.  tests/test_open_reference.py proves the reference (against the oracle route, scipy.linalg.expm and long
double: it agrees with them to 1e-14 or better) and that the shared comparison notices a subtly wrong side.

Signals are O(1) (open_helpers.order_one_states): every case asserts ON THE REFERENCE ALONE min_k |tau_k| >= 0.1 and
||G||_inf >= 1e-3, so the floor of tol_G never engages.  Tolerances are the project's, on every output:
    |dJ| <= 1e-12,  |dtau_k| <= 1e-12,  ||dG||_inf <= 1e-10 ||G||_inf,  ||d rho(T)||_inf <= 1e-12,  ||d tau_grads||_inf <= 1e-12
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
import open_reference as orf  # noqa: E402
from open_helpers import TOL_J, TOL_TAU, tol_G  # noqa: E402

pytestmark = pytest.mark.gpu

SM, SS, RE = 0, 1, 2
THETA = 3.0   # sub-step threshold of the kernels


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


# name -> d, J, L, K, functional, extras.  NP = 16 ceil(d / 16); every NP sees every functional.  Eight collapse operators mix
# the state quickly, which makes the gradient small: where the target of the pulse 0.8 x left ||G||_inf below 1e-3 the case
# takes the target of the pulse -0.8 x, and the rows with a long interval a base step of 0.5.
CASES = {
    "d17_J8_L3_K3_sm": dict(d=17, J=8, L=3, K=3, functional=SM, weights=True, shape=True, nonuniform=True, factor=-0.8),
    "d31_J1_L1_K2_ss": dict(d=31, J=1, L=1, K=2, functional=SS, hermitian=False, non_hermitian_states=0.3),
    "d32_J4_L2_K2_re": dict(d=32, J=4, L=2, K=2, functional=RE, cops_per_traj=True),
    "d33_J7_L5_K2_ss": dict(d=33, J=7, L=5, K=2, functional=SS, shape=True),
    "d47_J0_L2_K3_sm": dict(d=47, J=0, L=2, K=3, functional=SM, hc_per_traj=True),
    "d48_J8_L1_K1_re": dict(d=48, J=8, L=1, K=1, functional=RE, long_step=6.0, dt=0.5, factor=-0.8),
    "d49_J5_L3_K2_sm": dict(d=49, J=5, L=3, K=2, functional=SM, weights=True, cops_per_traj=True),
    "d63_J2_L2_K3_ss": dict(d=63, J=2, L=2, K=3, functional=SS, hermitian=False, non_hermitian_states=0.3,
                            non_hermitian_controls=True),
    "d64_J8_L2_K2_re": dict(d=64, J=8, L=2, K=2, functional=RE, weights=True, shape=True, factor=-0.8),
    "d64_J8_L4_K1_sm": dict(d=64, J=8, L=4, K=1, functional=SM, long_step=4.0, dt=0.5, factor=-0.8),
    "d16_J8_L1_K3_ss": dict(d=16, J=8, L=1, K=3, functional=SS, weights=True, shape=True, nonuniform=True, factor=-0.8),
    "d12_J8_L3_K3_re": dict(d=12, J=8, L=3, K=3, functional=RE, weights=True, shape=True, nonuniform=True),
    "d16_J8_L3_K3_sm": dict(d=16, J=8, L=3, K=3, functional=SM, weights=True, shape=True, nonuniform=True, factor=-0.8),
    # the further checks at NP > 16 (not evaluated as rows of the table)
    "shards_d48": dict(d=48, J=2, L=2, K=4, functional=SM, weights=True, shape=True, nonuniform=True),
}
TABLE = [name for name in CASES if name[0] == "d"]


def build_case(name):
    from grape_jl_amd import synth
    c = CASES[name]
    d, J, L, K, N_T = c["d"], c["J"], c["L"], c["K"], c.get("N_T", 3)
    seed = 1000 * d + 10 * J + L
    pr = synth.make_open_problem(d, L, N_T, K, J, seed=seed, cops_per_traj=c.get("cops_per_traj", False),
                                 hermitian=c.get("hermitian", True))
    rng = np.random.default_rng(seed)
    dts = rng.uniform(0.5, 1.5, N_T) if c.get("nonuniform") else np.full(N_T, c.get("dt", 1.0))
    if c.get("long_step"):
        dts[1] *= c["long_step"]
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(dts)])
    pr["shape"] = rng.uniform(0.5, 1.0, (L, N_T)) if c.get("shape") else None
    pr["weights"] = np.array([0.5, 1.0, 1.5, 0.8])[:K] if c.get("weights") else None
    if c.get("hc_per_traj"):
        pr["Hc"] = np.stack([(1.0 + 0.3 * k) * pr["Hc"][::(-1 if k % 2 else 1)] for k in range(K)])
    if c.get("non_hermitian_controls"):
        z = synth.normal(synth.subseed(seed, 9000), 2 * L * d * d).reshape(2, L, d, d)
        pr["Hc"] = pr["Hc"] + 0.1 / np.sqrt(d) * (z[0] + 1j * z[1])
    pr["functional"] = c["functional"]
    return oh.order_one_states(pr, seed, factor=c.get("factor", 0.8), non_hermitian=c.get("non_hermitian_states", 0.0))


_CACHE = {}


def reference_of(name):
    """(problem, propagate() parts) of a case: computed once, shared, never modified"""
    if name not in _CACHE:
        pr = build_case(name)
        _CACHE[name] = (pr, orf.propagate(pr, pr["pulsevals"]))
    return _CACHE[name]


def want_of(name, functional=None):
    pr, parts = reference_of(name)
    want = orf.from_parts(parts, pr, pr["functional"] if functional is None else functional)
    oh.assert_order_one(want)
    return pr, want


def _open(g, pr, functional=None, **kw):
    return g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr.get("target"), pr.get("weights"),
                          functional=pr["functional"] if functional is None else functional, shape=pr.get("shape"), **kw)


def _outputs(h, x):
    J, G, tau, rhoT = h.eval(x, want_psiT=True)
    return dict(J=J, G=G, tau=tau, rhoT=rhoT, tau_grads=h.tau_grads())


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[key]), np.asarray(b[key])) for key in ("J", "G", "tau", "rhoT", "tau_grads"))


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE)
def test_against_the_matrix_form_reference(g, name):
    pr, want = want_of(name)
    with _open(g, pr) as h:
        got = _outputs(h, pr["pulsevals"])
        work = h.work()
    oh.assert_open_agrees(got, want, name)
    N_T, K = len(pr["tlist"]) - 1, pr["H0"].shape[0]
    if CASES[name].get("long_step"):
        assert work["series_steps"] > 2 * K * N_T
    else:
        assert work["series_steps"] >= 2 * K * N_T


# ---- plumbing at NP > 16 ----------------------------------------------------------------------------------------------------
def test_backward_chi_at_d64_J8(g):
    """the chi of the built-in functional through grape_backward_chi, with and without a target in the handle"""
    name = "d64_J8_L2_K2_re"
    pr, want = want_of(name)
    K, w = 2, pr["weights"]
    for functional in (SM, SS, RE):
        _, want = want_of(name, functional)
        f = np.sum(w * want["tau"])
        chi = [w * f / K ** 2, w * want["tau"] / K, w / (2.0 * K) + 0j][functional][:, None, None] * pr["target"]
        with _open(g, pr, functional) as h:
            h.forward(pr["pulsevals"])
            Gc = h.backward_chi(chi)
            tg = h.tau_grads()
        oh.assert_open_agrees(dict(G=Gc, tau_grads=tg), dict(G=want["G"], tau_grads=want["tau_grads"]), f"chi {functional}")
    with _open(g, dict(pr, target=None), RE) as h:
        with pytest.raises(g.GrapeHipError):
            h.eval(pr["pulsevals"])
        h.forward(pr["pulsevals"])
        rhoT = h.final_states()
        Gn = h.backward_chi(chi)
        tgn = h.tau_grads()
    oh.assert_open_agrees(dict(G=Gn, rhoT=rhoT, tau_grads=tgn), dict(G=want["G"], rhoT=want["rhoT"], tau_grads=want["tau_grads"]),
                          "no target")
    assert np.array_equal(Gn, Gc) and np.array_equal(tgn, tg)      # the same chi: the same bits


@pytest.mark.parametrize("functional", [SM, SS, RE], ids=["sm", "ss", "re"])
def test_two_shards_at_d48(g, functional):
    pr, want = want_of("shards_d48", functional)
    x = pr["pulsevals"]
    parts = []
    for s in (slice(0, 2), slice(2, 4)):
        sub = dict(pr, H0=pr["H0"][s], rho0=pr["rho0"][s], target=pr["target"][s], weights=pr["weights"][s])
        parts.append(_open(g, sub, functional, K_total=4))
    try:
        taus = [h.forward(x) for h in parts]
        sums = sum(h.sums() for h in parts)
        f = complex(sums[0], sums[1])
        Gs = sum(h.backward(f) for h in parts)
        tg = np.concatenate([h.tau_grads() for h in parts])
        rhoT = np.concatenate([h.final_states() for h in parts])
    finally:
        for h in parts:
            h.close()
    Js = [1 - abs(f) ** 2 / 16, 1 - sums[2] / 4, 1 - sums[3] / 4][functional]
    oh.assert_open_agrees(dict(J=Js, G=Gs, tau=np.concatenate(taus), rhoT=rhoT, tau_grads=tg), want, "shards")


def test_set_tlist_at_d33(g):
    name = "d33_J7_L5_K2_ss"
    pr, want = want_of(name)
    rng = np.random.default_rng(33)
    t2 = np.concatenate([[0.0], np.cumsum(rng.uniform(0.4, 1.6, 3))])
    want2 = orf.evaluate(pr, pr["pulsevals"], functional=SS, tlist=t2)
    oh.assert_order_one(want2)
    with _open(g, pr) as h:
        first = _outputs(h, pr["pulsevals"])
        h.set_tlist(t2)
        moved = _outputs(h, pr["pulsevals"])
    with _open(g, dict(pr, tlist=t2)) as h:
        fresh = _outputs(h, pr["pulsevals"])
    oh.assert_open_agrees(first, want, "first grid")
    oh.assert_open_agrees(moved, want2, "second grid")
    assert _same_bits(moved, fresh)
    assert moved["J"] != first["J"]


# ---- splitting an interval ----------------------------------------------------------------------------------------------
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
    """Interval 1 replaced by two of half the length with the same pulse value: the same J, tau, rho(T), and G_1 = G_1' +
    G_1''.  beta dt / theta of the whole interval lies just below 2 (two sub-steps against 1 + 1: the same arithmetic steps,
    through another loop) or just above (three sub-steps of dt / 3 against 2 + 2 of dt / 4)."""
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
        J, G, tau, rhoT = h.eval(x, want_psiT=True)
        steps = h.work()["series_steps"]
    with _open(g, dict(pr, tlist=tl_split), SM) as h:
        Js, Gs, taus, rhoTs = h.eval(x2, want_psiT=True)
        steps_split = h.work()["series_steps"]
    assert steps == 2 * K * (2 + sub_whole) and steps_split == 2 * K * (2 + 2 * sub_halves)
    Gs = Gs.reshape(L, N_T + 1)
    Gm = np.stack([Gs[:, 0], Gs[:, 1] + Gs[:, 2], Gs[:, 3]], axis=1).reshape(-1)
    assert np.abs(tau).min() >= 0.1 and np.abs(G).max() >= 1e-3
    oh.assert_open_agrees(dict(J=Js, G=Gm, tau=taus, rhoT=rhoTs), dict(J=J, G=G, tau=tau, rhoT=rhoT), f"split d={d}")


# ---- error paths: defined returns ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [17, 64])
def test_a_hopeless_interval_is_an_error_and_the_handle_recovers(g, d):
    """beta dt > 4096 theta 30: the sub-step count is clamped at 4096, the first series runs into the 200-term limit, and
    every later one is cut after one term, so the sweep ends quickly: GRAPE_ERR_TAYLOR with a message from eval; back on the
    sane grid the handle gives its first result bit for bit"""
    from grape_jl_amd import synth
    pr = synth.make_open_problem(d, 2, 3, 2, 2, seed=900 + d)
    pr["functional"] = SM
    bad = pr["tlist"].copy()
    bad[2:] += 1e6 - 1.0       # beta >= 2: beta dt / theta >= 6.7e5 > 4096 * 30
    with _open(g, pr) as h:
        first = _outputs(h, pr["pulsevals"])
        h.set_tlist(bad)
        with pytest.raises(g.GrapeHipError) as err:
            h.eval(pr["pulsevals"])
        assert err.value.code == -5                                 # GRAPE_ERR_TAYLOR
        assert "did not converge" in str(err.value)
        h.set_tlist(pr["tlist"])
        again = _outputs(h, pr["pulsevals"])
        h.check()
    assert _same_bits(first, again)


@pytest.mark.parametrize("d", [5, 40])
def test_a_zero_weight_under_ss_behaves_as_on_the_closed_path(g, d):
    """weights = [0, 1] under J_T_ss: chi_0(T) = 0.  The open kernels must return what the closed path returns on a small
    closed problem with the same weights; after an error the handle stays usable."""
    from grape_jl_amd import synth
    w = np.array([0.0, 1.0])

    def status(h, x):
        try:
            h.eval(x)
            return 0
        except g.GrapeHipError as e:
            return e.code

    cl = synth.make_problem(5, 2, 3, 2, seed=77)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"], w, functional=SS) as hc:
        rc_closed = status(hc, cl["pulsevals"])
    pr = synth.make_open_problem(d, 2, 3, 2, 2, seed=910 + d)
    pr["functional"], pr["weights"] = SS, w
    oh.order_one_states(pr, 910 + d)
    want = orf.evaluate(pr, pr["pulsevals"], functional=SS)
    with _open(g, pr) as h:
        rc_open = status(h, pr["pulsevals"])
        print(dict(closed=rc_closed, open=rc_open))
        assert rc_open == rc_closed
        if rc_open != 0:
            assert rc_open == -3                                    # GRAPE_ERR_CHI_NORM
            assert b"chi_min_norm" in h._lib.grape_last_error(h._h)
        # usable: the forward half, and a backward sweep from a chi that is not zero
        J, _, tau = h.eval(pr["pulsevals"], gradient=False)
        assert abs(J - want["J"]) <= TOL_J and np.abs(tau - want["tau"]).max() <= TOL_TAU
        h.forward(pr["pulsevals"])
        chi = (np.array([1.0, 1.0]) * want["tau"] / 2)[:, None, None] * pr["target"]
        G1 = h.backward_chi(chi)
    want1 = orf.evaluate(pr, pr["pulsevals"], functional=SS, weights=np.ones(2))
    assert np.abs(G1 - want1["G"]).max() <= tol_G(want1["G"])


# ---- long-double pins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", [SM, SS, RE], ids=["sm", "ss", "re"])
@pytest.mark.parametrize("name", ["d33", "d48", "d64"])
def test_long_double_pins(g, name, functional):
    """tests/golden/open_pin_<name>.json (tests/golden/make_open_pins.py): the reference in x87 long double"""
    if ("pin", name) not in _CACHE:
        _CACHE[("pin", name)] = oh.load_open_pin(name)
    pr, want = _CACHE[("pin", name)]
    w = want[functional]
    oh.assert_order_one(w)
    with _open(g, pr, functional) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        tg = h.tau_grads()
    oh.assert_open_agrees(dict(J=J, G=G, tau=tau, tau_grads=tg), w, f"pin {name} {functional}")
