"""State running costs on open-system handles (grape_open_set_running_cost, grape_open_backward_xi;
csrc/grape_lindblad_rc.hip.h) against the matrix-form reference of tests/open_runcost_reference.py -- needs an MI355X.
tests/test_open_runcost_reference.py proves the reference (against oracle/grape_oracle.py on the vectorised problem and against
long double: 1e-14) and that the shared comparison refuses seven subtly wrong references.

N_T = 3: the smallest grid with a skipped n = 0, two interior terms and the boundary.  Problems come from the recipe of
tests/test_gpu_open_reference.py (build_case), D is a random complex Hermitian matrix of unit 2-norm, and lambda_b is chosen FROM
THE REFERENCE ALONE as the power of two nearest ||G_T||_inf / ||G_b||_inf.  Every case asserts on the reference alone
min_k |tau_k| >= 0.1, ||G_T||_inf >= 1e-3, lambda_b ||G_b||_inf >= 1e-3 and ||G||_inf >= 1e-3, so ||dG||_inf <= 1e-10 ||G||_inf is
relative for both parts.  Tolerances are the project's (open_helpers.assert_open_agrees) plus |dJ_b| <= 1e-12.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
import open_runcost_reference as rcf  # noqa: E402
import test_gpu_open_reference as gor  # noqa: E402
from open_helpers import TOL_J, tol_G  # noqa: E402

pytestmark = pytest.mark.gpu

SM, SS, RE = 0, 1, 2
RUNNING_COST = "running cost"


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


# name -> the keys of test_gpu_open_reference.CASES, plus D_per_traj.  Every NP (16, 32, 48, 64), both wave layouts of the
# backward kernel (one tile per wave, two at NP = 64), padded (d = 5, 17, 33, 49) and full (16, 48, 64) tiles.
CASES = {
    "rc_d5_J1_L1_K2_sm": dict(d=5, J=1, L=1, K=2, functional=SM),
    "rc_d16_J8_L3_K3_ss": dict(d=16, J=8, L=3, K=3, functional=SS, D_per_traj=True, weights=True, shape=True, nonuniform=True,
                               factor=-0.8),
    "rc_d17_J2_L2_K2_re": dict(d=17, J=2, L=2, K=2, functional=RE),
    "rc_d33_J0_L1_K1_sm": dict(d=33, J=0, L=1, K=1, functional=SM, long_step=6.0, dt=0.5),
    "rc_d48_J3_L2_K2_ss": dict(d=48, J=3, L=2, K=2, functional=SS, D_per_traj=True),
    "rc_d49_J1_L3_K2_re": dict(d=49, J=1, L=3, K=2, functional=RE),
    "rc_d64_J8_L2_K2_sm": dict(d=64, J=8, L=2, K=2, functional=SM, weights=True, shape=True, nonuniform=True, long_step=3.0,
                               factor=-0.8),
    # the further checks (not evaluated as rows of the table)
    "rc_chi_d33": dict(d=33, J=2, L=2, K=2, functional=SS, weights=True),
    "rc_shards_d48": dict(d=48, J=2, L=2, K=4, functional=SM, D_per_traj=True, weights=True, shape=True, nonuniform=True),
}
TABLE = [name for name in CASES if name.startswith("rc_d")]


def build_case(name):
    """the recipe of tests/test_gpu_open_reference.py on a row of this file's table"""
    gor.CASES[name] = CASES[name]
    try:
        return gor.build_case(name)
    finally:
        del gor.CASES[name]


_CACHE = {}


def case_of(name):
    """(problem, D) of a case: built once, shared, never modified"""
    if ("case", name) not in _CACHE:
        pr = build_case(name)
        c = CASES[name]
        _CACHE[("case", name)] = (pr, rcf.hermitian_D(c["d"] * 100 + c["J"], c["d"], c["K"] if c.get("D_per_traj") else None))
    return _CACHE[("case", name)]


def want_of(name, functional=None, **cost):
    """(problem, D, lambda_b, reference outputs): the reference is computed once per (case, functional, cost), lambda_b comes
    from it, and the conditions on the signals are asserted on it alone"""
    pr, D = case_of(name)
    functional = pr["functional"] if functional is None else functional
    key = (name, functional, tuple(sorted(cost)))
    if key not in _CACHE:
        _CACHE[key] = rcf.evaluate(pr, pr["pulsevals"], functional=functional, lambda_b=1.0, **(cost or dict(D=D)))
    lam = rcf.lambda_from(_CACHE[key])
    want = rcf.with_lambda(_CACHE[key], lam)
    rcf.assert_order_one(want, lam)
    return pr, D, lam, want


PURITY = dict(g_b=lambda rho, k, m: -np.sum(np.abs(rho) ** 2), xi=lambda rho, k, m: rho)     # g_b = -tr(rho^dagger rho)


def _outputs(h, x):
    J, G, tau, rhoT = h.eval(x, want_psiT=True)
    return dict(J=J, G=G, tau=tau, rhoT=rhoT, tau_grads=h.tau_grads(), J_b=h.sums()[4])


def _same_bits(a, b, keys=("J", "G", "tau", "rhoT", "tau_grads", "J_b")):
    return all(np.array_equal(np.asarray(a[key]), np.asarray(b[key])) for key in keys)


def _xi_of(D, K, N_T):
    """the built-in family as a caller's xi: -D_k^dagger / 2 at every n, [K, N_T+1, d, d]"""
    D = np.asarray(D)
    Dk = np.broadcast_to(D, (K,) + D.shape[-2:])
    return np.ascontiguousarray(np.broadcast_to((-np.conj(np.swapaxes(Dk, -1, -2)) / 2)[:, None], (K, N_T + 1) + D.shape[-2:]))


def _message(h):
    return h._lib.grape_last_error(h._h).decode()


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLE)
def test_against_the_matrix_form_reference(g, name):
    pr, D, lam, want = want_of(name)
    with gor._open(g, pr) as h:
        h.set_running_cost(D, lam)
        got = _outputs(h, pr["pulsevals"])
        work = h.work()
    rcf.assert_runcost_agrees(got, want, name)
    N_T, K = len(pr["tlist"]) - 1, pr["H0"].shape[0]
    print(name, dict(series_steps=work["series_steps"]))
    if CASES[name].get("long_step"):
        assert work["series_steps"] > 2 * K * N_T       # an interval is cut: the inhomogeneity must come once per interval
    else:
        assert work["series_steps"] >= 2 * K * N_T


# ---- an independent kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [12, 64])
def test_pure_states_against_the_closed_path(g, d):
    """rho = |Psi><Psi|, no dissipation: tr(D rho) = <Psi|D|Psi> and tr(sigma rho(T)) = |<phi|Psi(T)>|^2, so the open handle under
    J_T_re with the cost is the closed handle under J_T_ss with Dpen and the same lambda_b and weights"""
    from grape_jl_amd import synth
    K = 2
    pr = synth.make_problem(d, 2, 3, K, seed=5200 + d)
    w = np.array([0.7, 1.3])
    D, lam = rcf.hermitian_D(5200 + d, d), 0.5
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], w, functional=g.J_T_SS, D=D, lambda_b=lam) as hc:
        Jc, Gc, tauc = hc.eval(pr["pulsevals"])
        Jbc = hc.sums()[4]
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], w, functional=g.J_T_SS) as hc_plain:
        G_plain = hc_plain.eval(pr["pulsevals"])[1]
    proj = lambda v: v[:, :, None] * v[:, None, :].conj()   # noqa: E731
    op = dict(H0=pr["H0"], Hc=pr["Hc"], cops=None, tlist=pr["tlist"], rho0=proj(pr["psi0"]), target=proj(pr["target"]), weights=w)
    with gor._open(g, op, functional=g.J_T_RE) as h:
        h.set_running_cost(D, lam)
        J, G, tau = h.eval(pr["pulsevals"])
        Jb = h.sums()[4]
    fig = dict(dJ=abs(J - Jc), dJb=abs(Jb - Jbc), dG=np.abs(G - Gc).max(), tolG=tol_G(Gc), cost_in_G=np.abs(Gc - G_plain).max())
    print(fig)
    assert fig["cost_in_G"] >= 1e-3                      # (the cost is visible in the closed gradient)
    assert fig["dJ"] <= TOL_J and fig["dJb"] <= rcf.TOL_JB and fig["dG"] <= fig["tolG"]


# ---- the caller's xi ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rc_d17_J2_L2_K2_re", "rc_d64_J8_L2_K2_sm"])
def test_the_built_in_family_as_a_callers_xi_gives_the_same_bits(g, name):
    pr, D, lam, want = want_of(name)
    K, N_T = pr["H0"].shape[0], len(pr["tlist"]) - 1
    with gor._open(g, pr) as h:
        h.set_running_cost(D, lam)
        _, G, _ = h.eval(pr["pulsevals"])
        tg = h.tau_grads()
        h.set_running_cost(None, 0.0)
        h.forward(pr["pulsevals"])
        G2 = h.open_backward_xi(_xi_of(D, K, N_T), lam)
        tg2 = h.tau_grads()
    assert np.abs(G - want["G"]).max() <= tol_G(want["G"])
    assert np.array_equal(G, G2) and np.array_equal(tg, tg2)


@pytest.mark.parametrize("name", ["rc_d17_J2_L2_K2_re", "rc_d49_J1_L3_K2_re"])
def test_the_purity_cost_through_the_callers_xi(g, name):
    """g_b = -tr(rho^dagger rho), xi = rho_k(t_n) read back from storage()"""
    pr, _, lam, want = want_of(name, **PURITY)
    with gor._open(g, pr) as h:
        tau = h.forward(pr["pulsevals"])
        st = h.storage()
        G = h.open_backward_xi(st, lam)
        got = dict(G=G, tau=tau, tau_grads=h.tau_grads(), rhoT=h.final_states(), J_b=float(np.sum(-np.sum(np.abs(st) ** 2, axis=(-2, -1)) @ rcf.trapezoid_weights(pr["tlist"]))))
    rcf.assert_runcost_agrees(got, want, name + " purity")


def test_the_callers_chi_with_and_without_targets_at_d33(g):
    name = "rc_chi_d33"
    pr, D, lam, want = want_of(name)
    K, N_T, w = 2, 3, pr["weights"]
    chi = (w * want["tau"] / K)[:, None, None] * pr["target"]            # chi of J_T_ss
    xi = _xi_of(D, K, N_T)
    with gor._open(g, pr) as h:
        h.forward(pr["pulsevals"])
        Gc = h.open_backward_xi(xi, lam, chi=chi)
        tg = h.tau_grads()
    rcf.assert_runcost_agrees(dict(G=Gc, tau_grads=tg), dict(G=want["G"], tau_grads=want["tau_grads"]), "chi, with targets")
    with gor._open(g, dict(pr, target=None)) as h:
        h.forward(pr["pulsevals"])
        rc = h._lib.grape_open_backward_xi(h._h, np.zeros(2).ctypes.data, None, xi.ctypes.data, lam, np.zeros(6).ctypes.data)
        assert rc == -1 and "no target" in _message(h)
        Gn = h.open_backward_xi(xi, lam, chi=chi)
        tgn = h.tau_grads()
    assert np.array_equal(Gn, Gc) and np.array_equal(tgn, tg)      # the same chi and xi: the same bits


def test_two_shards_at_d48(g):
    name = "rc_shards_d48"
    pr, D, lam, want = want_of(name)
    x = pr["pulsevals"]
    parts = []
    for s in (slice(0, 2), slice(2, 4)):
        sub = dict(pr, H0=pr["H0"][s], rho0=pr["rho0"][s], target=pr["target"][s], weights=pr["weights"][s])
        parts.append(gor._open(g, sub, K_total=4))
        parts[-1].set_running_cost(D[s], lam)
    try:
        taus = [h.forward(x) for h in parts]
        each = [h.sums() for h in parts]
        sums = sum(each)
        f = complex(sums[0], sums[1])
        Gs = sum(h.backward(f) for h in parts)
        tg = np.concatenate([h.tau_grads() for h in parts])
        rhoT = np.concatenate([h.final_states() for h in parts])
    finally:
        for h in parts:
            h.close()
    with gor._open(g, pr) as h:
        h.set_running_cost(D, lam)
        single = _outputs(h, x)
    Js = 1 - abs(f) ** 2 / 16 + lam * sums[4]
    got = dict(J=Js, G=Gs, tau=np.concatenate(taus), rhoT=rhoT, tau_grads=tg, J_b=sums[4])
    rcf.assert_runcost_agrees(got, want, "shards")
    rcf.assert_runcost_agrees(got, single, "shards against the single handle")
    assert abs(each[0][4] - np.sum(want["Jb_k"][:2])) <= rcf.TOL_JB and abs(each[1][4] - np.sum(want["Jb_k"][2:])) <= rcf.TOL_JB


# ---- state and refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rc_d17_J2_L2_K2_re", "rc_d64_J8_L2_K2_sm"])
def test_removal_repetition_new_grid_and_batch_are_bitwise(g, name):
    pr, D, lam, want = want_of(name)
    x = pr["pulsevals"]
    rng = np.random.default_rng(17)
    t2 = np.concatenate([[0.0], np.cumsum(rng.uniform(0.4, 1.6, 3))])
    with gor._open(g, pr) as h:
        fresh = _outputs(h, x)
    with gor._open(g, dict(pr, tlist=t2)) as h:
        h.set_running_cost(D, lam)
        fresh2 = _outputs(h, x)
    with gor._open(g, pr) as h:
        h.set_running_cost(D, lam)
        first = _outputs(h, x)
        again = _outputs(h, x)
        Jb, Gb, taub = h.eval_batch(np.stack([x, 0.5 * x, x]))
        h.set_tlist(t2)
        moved = _outputs(h, x)
        h.set_tlist(pr["tlist"])
        h.set_running_cost(None, 0.0)
        removed = _outputs(h, x)
        h.set_running_cost(D, 2 * lam)                     # (a continuation in lambda_b)
        doubled = _outputs(h, x)
    rcf.assert_runcost_agrees(first, want, name)
    assert _same_bits(first, again)
    assert Jb[0] == first["J"] and Jb[2] == first["J"] and np.array_equal(Gb[0], first["G"]) and np.array_equal(Gb[2], first["G"])
    assert np.array_equal(taub[0], first["tau"]) and Jb[1] != Jb[0]
    assert _same_bits(moved, fresh2) and moved["J"] != first["J"]
    assert _same_bits(removed, fresh) and removed["J_b"] == 0.0 and fresh["J"] != first["J"]
    rcf.assert_runcost_agrees(doubled, rcf.with_lambda(want, 2 * lam), name + " 2 lambda")


def test_kernels_that_do_not_carry_the_cost_refuse_it(g):
    name = "rc_d17_J2_L2_K2_re"
    pr, D, lam, want = want_of(name)
    x = pr["pulsevals"]
    K, N_T = pr["H0"].shape[0], len(pr["tlist"]) - 1
    with gor._open(g, pr) as h:
        h.set_running_cost(D, lam)
        first = _outputs(h, x)
        for call in (h.time_gradient, lambda: h.open_hvp(np.ones_like(x)), lambda: h.open_eval_batch(x[None])):
            with pytest.raises(g.GrapeHipError) as err:
                call()
            assert err.value.code == -1 and RUNNING_COST in str(err.value), str(err.value)
            assert _same_bits(_outputs(h, x), first)
        # a backward half without a cost makes the time gradient answer again; a caller's xi withdraws it once more
        h.set_running_cost(None, 0.0)
        with pytest.raises(g.GrapeHipError) as err:
            h.time_gradient()
        assert "grape_open_set_running_cost" in str(err.value)
        plain = _outputs(h, x)
        dJdt = h.time_gradient()
        h.open_hvp(np.ones_like(x))
        h.open_backward_xi(_xi_of(D, K, N_T), lam)
        with pytest.raises(g.GrapeHipError) as err:
            h.time_gradient()
        assert err.value.code == -1 and RUNNING_COST in str(err.value)
        h.backward(complex(*h.sums()[:2]))
        assert np.array_equal(h.time_gradient(), dJdt)
    with gor._open(g, pr) as h:
        fresh = _outputs(h, x)
        assert np.array_equal(h.time_gradient(), dJdt)
    assert _same_bits(plain, fresh)


def test_defined_refusals_leave_the_handle_usable(g):
    from grape_jl_amd import synth
    name = "rc_d5_J1_L1_K2_sm"
    pr, D, lam, want = want_of(name)
    x = pr["pulsevals"]
    xi = _xi_of(D, 2, 3)
    p = np.zeros(8)
    cl = synth.make_problem(5, 1, 3, 2, seed=7)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"]) as hc:
        lib = hc._lib
        assert lib.grape_open_set_running_cost(hc._h, p.ctypes.data, 0, 0.5) == -1 and "not an open-system handle" in _message(hc)
        assert lib.grape_open_backward_xi(hc._h, p.ctypes.data, None, p.ctypes.data, 0.5, p.ctypes.data) == -1
        assert "grape_backward_xi" in _message(hc)
        hc.eval(cl["pulsevals"])
    with gor._open(g, pr) as h:
        Dc = np.ascontiguousarray(D.T)
        for bad in (np.inf, np.nan):
            assert lib.grape_open_set_running_cost(h._h, Dc.ctypes.data, 0, ctypes.c_double(bad)) == -1 and "finite" in _message(h)
        Gbuf = np.zeros(3)
        f = np.zeros(2)
        assert lib.grape_open_backward_xi(h._h, f.ctypes.data, None, xi.ctypes.data, lam, Gbuf.ctypes.data) == -1
        assert "no forward half" in _message(h)                                         # since create
        h.forward(x)
        assert lib.grape_open_backward_xi(h._h, f.ctypes.data, None, None, lam, Gbuf.ctypes.data) == -1 and "NULL" in _message(h)
        assert lib.grape_open_backward_xi(h._h, f.ctypes.data, None, xi.ctypes.data, lam, None) == -1 and "NULL" in _message(h)
        h.set_tlist(pr["tlist"])
        with pytest.raises(g.GrapeHipError, match="no forward half"):
            h.open_backward_xi(xi, lam, f_total=0j)
        h.forward(x)
        h.set_running_cost(D, lam)
        with pytest.raises(g.GrapeHipError, match="no forward half"):
            h.open_backward_xi(xi, lam, f_total=0j)
        with pytest.raises(g.GrapeHipError):
            h.backward(0j)                                                              # (grape_backward needs the forward half too)
        rcf.assert_runcost_agrees(_outputs(h, x), want, "after the refusals")


def test_a_zero_weight_under_ss_has_a_chi_once_a_cost_is_set(g):
    """weights = [0, 1] under J_T_ss: chi_0(T) = 0 without a cost (GRAPE_ERR_CHI_NORM,
    test_gpu_open_reference.test_a_zero_weight_under_ss_behaves_as_on_the_closed_path); with one chi_0(T) = lambda_b wq xi_0(T)"""
    name = "rc_d17_J2_L2_K2_re"
    pr, D = case_of(name)
    pr = dict(pr, weights=np.array([0.0, 1.0]))
    want1 = rcf.evaluate(pr, pr["pulsevals"], functional=SS, D=D, lambda_b=1.0)
    lam = rcf.lambda_from(want1)
    want = rcf.with_lambda(want1, lam)
    rcf.assert_order_one(want, lam)
    with gor._open(g, pr, SS) as h:
        with pytest.raises(g.GrapeHipError) as err:
            h.eval(pr["pulsevals"])
        assert err.value.code == -3                                 # GRAPE_ERR_CHI_NORM
        h.set_running_cost(D, lam)
        got = _outputs(h, pr["pulsevals"])                          # GRAPE_OK
    rcf.assert_runcost_agrees(got, want, "w = [0, 1]")
