"""Open-system handles (grape_create_open / GrapeHipOpen): d x d density matrices under a Lindblad generator, propagated in
matrix form -- needs an MI355X.

References: the C oracle on the VECTORISED problem (built in tests/open_helpers.py with numpy.kron; exact up to d = 16, and
through a product construction up to d = 64), the closed path of this library on the product's ``liouvillian()`` and on
pure states, finite differences, and the invariants of a density matrix.  Tolerances are the project's:
    |dJ| <= 1e-12,   |dtau_k| <= 1e-12,   ||dG||_inf <= 1e-10 * max(||G||_inf, 1e-3)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
from open_helpers import TOL_J, TOL_TAU, tol_G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


def _case(d, J, N_T=6, K=3, seed=None, cops_per_traj=False, hermitian=True, long_step=None):
    """K = 3 with weights, a shape and a non-uniform grid"""
    from grape_jl_amd import synth
    pr = synth.make_open_problem(d, 2, N_T, K, J, seed=(100 * d + J) if seed is None else seed, cops_per_traj=cops_per_traj,
                                 hermitian=hermitian)
    rng = np.random.default_rng(1000 + 10 * d + J)
    dts = rng.uniform(0.5, 1.5, N_T)
    if long_step is not None:
        dts[long_step] *= 40.0
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(dts)])
    pr["shape"] = rng.uniform(0.5, 1.0, (2, N_T))
    pr["weights"] = np.array([0.5, 1.0, 1.5])[:K]
    return pr


def _open(g, pr, functional=0, **kw):
    return g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr.get("target"), pr.get("weights"),
                          functional=functional, shape=pr.get("shape"), **kw)


def _check_against_oracle(g, ref, pr, functional):
    want = oh.oracle(ref, pr, pr["pulsevals"], functional=functional, weights=pr["weights"], shape=pr["shape"])
    with _open(g, pr, functional) as h:
        J, G, tau, rhoT = h.eval(pr["pulsevals"], want_psiT=True)
        tg = h.tau_grads()
        work = h.work()
    figures = dict(dJ=abs(J - want["J"]), dtau=np.abs(tau - want["tau"]).max(), dG=np.abs(G - want["G"]).max(), tolG=tol_G(want["G"]),
                   drho=np.abs(rhoT - want["rhoT"]).max(), dtg=np.abs(tg - want["tau_grads"]).max())
    print(figures)
    assert figures["dJ"] <= TOL_J
    assert figures["dtau"] <= TOL_TAU
    assert figures["dG"] <= figures["tolG"]
    assert figures["drho"] <= 1e-12
    assert figures["dtg"] <= 1e-12
    return work


# ---- 5. the oracle, directly --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", [0, 1, 2], ids=["sm", "ss", "re"])
@pytest.mark.parametrize("J", [0, 1, 3])
@pytest.mark.parametrize("d", [2, 3, 5, 8, 12, 16])
def test_oracle_on_the_vectorised_problem(g, ref, d, J, functional):
    _check_against_oracle(g, ref, _case(d, J), functional)


def test_oracle_collapse_operators_per_trajectory(g, ref):
    _check_against_oracle(g, ref, _case(5, 2, cops_per_traj=True), 0)


def test_oracle_non_hermitian_drift_and_states(g, ref):
    pr = _case(8, 1, hermitian=False)
    rng = np.random.default_rng(3)
    pr["rho0"] = pr["rho0"] + 0.1 * (rng.normal(size=pr["rho0"].shape) + 1j * rng.normal(size=pr["rho0"].shape))
    pr["target"] = pr["target"] + 0.1j * rng.normal(size=pr["target"].shape)
    _check_against_oracle(g, ref, pr, 1)


def test_oracle_control_operators_per_trajectory(g, ref):
    pr = _case(3, 1)
    pr["Hc"] = np.stack([pr["Hc"], 1.3 * pr["Hc"], 0.7 * pr["Hc"]])
    _check_against_oracle(g, ref, pr, 2)


# ---- 9. sub-steps -------------------------------------------------------------------------------------------------------
def test_one_long_interval_is_sub_stepped(g, ref):
    pr = _case(8, 1, long_step=2)
    work = _check_against_oracle(g, ref, pr, 0)
    N_T, K = len(pr["tlist"]) - 1, 3
    assert work["series_steps"] > N_T
    # [8] counts the (sub-)steps of the K forward sweeps and of the K backward chi chains: without sub-steps 2 K N_T
    assert work["series_steps"] > 2 * K * N_T


# ---- 6. beyond d = 16, exactly: two uncoupled subsystems ----------------------------------------------------------------
def _factor(d, seed, N_T):
    from grape_jl_amd import synth
    pr = synth.make_open_problem(d, 1, N_T, 1, 1, seed=seed, gamma=0.05)
    pr["H0"] = 0.5 * pr["H0"]
    pr["Hc"] = 0.5 * pr["Hc"]
    return pr


@pytest.mark.parametrize("dA,dB", [(3, 8), (4, 8), (5, 8), (6, 8), (8, 8)])
def test_product_of_two_uncoupled_subsystems(g, ref, dA, dB):
    """H = H_A (x) 1 + 1 (x) H_B, one control and one collapse operator local to each side, rho(0) = rho_A (x) rho_B,
    sigma = sigma_A (x) sigma_B, all Hermitian: tau = tau_A tau_B, and under J_T_re with K = 1 the gradient with respect to
    the control of A is G_A tau_B (and vice versa).  The factors come from two oracle runs at d^2 <= 64; the library sees a
    dense d x d problem (d = 24, 32, 40, 48, 64: every padding, and the non-multiples of 16)."""
    N_T = 200
    A, B = _factor(dA, 11 + dA, N_T), _factor(dB, 77 + dA, N_T)
    rng = np.random.default_rng(dA)
    tlist = np.concatenate([[0.0], np.cumsum(rng.uniform(0.3, 1.5, N_T))])   # ||H|| ~ 1
    A["tlist"] = B["tlist"] = tlist
    eA, eB = np.eye(dA), np.eye(dB)
    xA, xB = A["pulsevals"], 0.7 * B["pulsevals"][::-1].copy()
    full = dict(H0=(np.kron(A["H0"][0], eB) + np.kron(eA, B["H0"][0]))[None],
                Hc=np.stack([np.kron(A["Hc"][0], eB), np.kron(eA, B["Hc"][0])]),
                cops=np.stack([np.kron(A["cops"][0], eB), np.kron(eA, B["cops"][0])]),
                rho0=np.kron(A["rho0"][0], B["rho0"][0])[None], target=np.kron(A["target"][0], B["target"][0])[None],
                tlist=tlist)
    oA = oh.oracle(ref, A, xA, functional=2)
    oB = oh.oracle(ref, B, xB, functional=2)
    tA, tB = oA["tau"][0], oB["tau"][0]
    assert abs(tA.imag) <= 1e-14 and abs(tB.imag) <= 1e-14
    want_tau = tA * tB
    want_G = np.concatenate([oA["G"] * tB.real, oB["G"] * tA.real])
    with _open(g, full, functional=2) as h:
        J, G, tau = h.eval(np.concatenate([xA, xB]))
    figures = dict(dtau=abs(tau[0] - want_tau), dJ=abs(J - (1.0 - want_tau.real)), dG=np.abs(G - want_G).max(), tolG=tol_G(want_G))
    print(figures)
    assert figures["dtau"] <= TOL_TAU
    assert figures["dJ"] <= TOL_J
    assert figures["dG"] <= figures["tolG"]


# ---- 7. a second implementation on the GPU: the closed path on liouvillian() ---------------------------------------------
@pytest.mark.parametrize("d", [4, 8, 16])
def test_vectorised_route_of_the_same_library(g, d):
    pr = _case(d, 2)
    Hv = np.stack([g.liouvillian(pr["H0"][k], pr["cops"]) for k in range(3)])
    Hcv = np.stack([g.liouvillian(pr["Hc"][l]) for l in range(2)])
    with g.GrapeHip(Hv, Hcv, pr["tlist"], oh.vec(pr["rho0"]), oh.vec(pr["target"]), pr["weights"], functional=0,
                    shape=pr["shape"]) as hv:
        Jv, Gv, tauv = hv.eval(pr["pulsevals"])
    with _open(g, pr, 0) as h:
        J, G, tau = h.eval(pr["pulsevals"])
    figures = dict(dJ=abs(J - Jv), dtau=np.abs(tau - tauv).max(), dG=np.abs(G - Gv).max(), tolG=tol_G(Gv))
    print(figures)
    assert figures["dJ"] <= 2 * TOL_J
    assert figures["dtau"] <= 2 * TOL_TAU
    assert figures["dG"] <= 2 * figures["tolG"]


# ---- 8. coupled, full size, against the headline path --------------------------------------------------------------------
def test_full_size_against_the_closed_path_and_invariants(g):
    from grape_jl_amd import synth
    d, N_T = 64, 300
    pr = synth.make_problem(d, 2, N_T, 1, seed=4242)
    psi, phi = pr["psi0"][0], pr["target"][0]
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], functional=g.J_T_SS) as hc:
        Jc, Gc, tauc = hc.eval(pr["pulsevals"])
    op = dict(H0=pr["H0"], Hc=pr["Hc"], cops=None, tlist=pr["tlist"], rho0=np.outer(psi, psi.conj())[None],
              target=np.outer(phi, phi.conj())[None])
    with _open(g, op, functional=g.J_T_RE) as h:
        J, G, tau = h.eval(pr["pulsevals"])
    figures = dict(dtau=abs(tau[0] - abs(tauc[0]) ** 2), dJ=abs(J - Jc), dG=np.abs(G - Gc).max(), tolG=tol_G(Gc))
    print(figures)
    assert figures["dtau"] <= TOL_TAU
    assert figures["dJ"] <= TOL_J
    assert figures["dG"] <= figures["tolG"]
    # the same problem with two collapse operators: finite differences and the invariants of a density matrix
    z = synth.normal(99, 2 * 2 * d * d)
    op["cops"] = np.sqrt(0.02 / d) * (z[0::2] + 1j * z[1::2]).reshape(2, d, d)
    with _open(g, op, functional=g.J_T_RE) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        st = h.storage()[0]
        eps = 1e-5
        for idx in (0, 37, 150, 299, 300, 300 + 111, 300 + 222, 599):
            xp, xm = pr["pulsevals"].copy(), pr["pulsevals"].copy()
            xp[idx] += eps
            xm[idx] -= eps
            fd = (h.eval(xp, gradient=False)[0] - h.eval(xm, gradient=False)[0]) / (2 * eps)
            print(idx, fd, G[idx])
            assert abs(fd - G[idx]) <= 5e-10 + 1e-5 * abs(G[idx])
    tr = np.trace(st, axis1=-2, axis2=-1)
    herm = np.abs(st - np.conj(np.swapaxes(st, -1, -2))).max()
    lam = np.linalg.eigvalsh(0.5 * (st + np.conj(np.swapaxes(st, -1, -2)))).min()
    print(dict(trace=np.abs(tr - 1.0).max(), herm=herm, lam_min=lam))
    assert np.abs(tr - 1.0).max() <= 1e-12
    assert herm <= 1e-12
    assert lam >= -1e-12


# ---- 10. plumbing --------------------------------------------------------------------------------------------------------
def test_backward_chi_reproduces_the_built_in_functional(g):
    pr = _case(5, 2)
    for functional in (0, 1, 2):
        with _open(g, pr, functional) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            K, w = 3, pr["weights"]
            f = np.sum(w * tau)
            coeff = [w * f / K ** 2, w * tau / K, w / (2.0 * K) + 0j][functional]
            h.forward(pr["pulsevals"])
            Gc = h.backward_chi(coeff[:, None, None] * pr["target"])
        assert np.abs(Gc - G).max() <= tol_G(G)


def test_no_target_works_through_the_chi_route(g):
    pr = _case(5, 2)
    with _open(g, pr, 2) as h:
        J, G, tau = h.eval(pr["pulsevals"])
    nt = dict(pr, target=None)
    with _open(g, nt, 2) as h:
        with pytest.raises(g.GrapeHipError):
            h.eval(pr["pulsevals"])
        h.forward(pr["pulsevals"])
        rhoT = h.final_states()
        tau2 = np.einsum("kij,kij->k", pr["target"].conj(), rhoT)
        assert np.abs(tau2 - tau).max() <= TOL_TAU
        Gc = h.backward_chi((pr["weights"] / 6.0)[:, None, None] * pr["target"])
    assert np.abs(Gc - G).max() <= tol_G(G)


def test_two_shards_add_up_to_the_single_handle(g):
    pr = _case(6, 2, K=3)
    from grape_jl_amd import synth
    big = synth.make_open_problem(6, 2, 6, 4, 2, seed=31)
    big["tlist"], big["shape"], big["weights"] = pr["tlist"], pr["shape"], np.array([0.5, 1.0, 1.5, 0.8])
    for functional in (0, 1, 2):
        with _open(g, big, functional) as h:
            J, G, tau = h.eval(big["pulsevals"])
        parts = []
        for s in (slice(0, 2), slice(2, 4)):
            sub = dict(big, H0=big["H0"][s], rho0=big["rho0"][s], target=big["target"][s], weights=big["weights"][s])
            parts.append(_open(g, sub, functional, K_total=4))
        taus = [h.forward(big["pulsevals"]) for h in parts]
        sums = sum(h.sums() for h in parts)
        f = complex(sums[0], sums[1])
        Gs = sum(h.backward(f) for h in parts)
        for h in parts:
            h.close()
        assert np.abs(np.concatenate(taus) - tau).max() <= TOL_TAU
        Js = [1 - abs(f) ** 2 / 16, 1 - sums[2] / 4, 1 - sums[3] / 4][functional]
        assert abs(Js - J) <= TOL_J
        assert np.abs(Gs - G).max() <= tol_G(G)


def test_set_tlist_batch_and_repeatability_are_bitwise(g):
    pr = _case(7, 2)
    rng = np.random.default_rng(8)
    t2 = np.concatenate([[0.0], np.cumsum(rng.uniform(0.4, 1.2, 6))])
    with _open(g, pr, 0) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        J1, G1, tau1 = h.eval(pr["pulsevals"])
        assert J1 == J and np.array_equal(G1, G) and np.array_equal(tau1, tau)
        # three pulse vectors in one call: the loop route, bit for bit three calls
        X = np.stack([pr["pulsevals"], 0.5 * pr["pulsevals"], pr["pulsevals"][::-1]])
        Jb, Gb, taub = h.eval_batch(X)
        assert h.batch_info()["route"] == 0
        for p in range(3):
            Jp, Gp, taup = h.eval(X[p])
            assert Jb[p] == Jp and np.array_equal(Gb[p], Gp) and np.array_equal(taub[p], taup)
        h.set_tlist(t2)
        Jt, Gt, taut = h.eval(pr["pulsevals"])
    with _open(g, dict(pr, tlist=t2), 0) as h:
        Jf, Gf, tauf = h.eval(pr["pulsevals"])
    assert Jt == Jf and np.array_equal(Gt, Gf) and np.array_equal(taut, tauf)
    assert Jt != J


def test_refused_calls_leave_the_handle_usable(g):
    import ctypes
    pr = _case(4, 1)
    with _open(g, pr, 0) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        lib, hd = h._lib, h._h
        buf = np.zeros(4 * 7 * 16 * 2 + 64)
        p = buf.ctypes.data
        calls = [("grape_get_propagator", lambda: lib.grape_get_propagator(hd, 0, 0, p)),
                 ("grape_get_storage", lambda: lib.grape_get_storage(hd, 1, p)),
                 ("grape_backward_xi", lambda: lib.grape_backward_xi(hd, p, None, p, ctypes.c_double(0.1), p)),
                 ("grape_get_time_gradient", lambda: lib.grape_get_time_gradient(hd, p)),
                 ("grape_forward_device", lambda: lib.grape_forward_device(hd, p, p, None)),
                 ("grape_backward_device", lambda: lib.grape_backward_device(hd, p, p, None))]
        for name, call in calls:
            assert call() == -1, name
            msg = lib.grape_last_error(hd)
            assert name.encode() in msg and b"open-system" in msg, (name, msg)
            J2, G2, tau2 = h.eval(pr["pulsevals"])
            assert J2 == J and np.array_equal(G2, G) and np.array_equal(tau2, tau), name
        h.check()
        assert h.set_fused_sweeps(True) is False
        t = h.timings()
        assert t["forward"] > 0.0 and t["backward"] > 0.0
        h.reset_timings()
        assert h.timings()["forward"] == -1.0
        w = h.work()
        assert w["cells"] == 3 * 6 and w["series_terms"] > 0 and w["mfma_flop_forward"] > 0 and w["mfma_flop_backward"] > 0


# ---- 11. reach -----------------------------------------------------------------------------------------------------------
def test_reach_d64_1000_steps_beside_a_closed_handle(g):
    from grape_jl_amd import synth
    c3 = synth.make_config("C3")
    op = synth.make_open_config("O64R")
    with g.GrapeHip(c3["H0"], c3["Hc"], c3["tlist"], c3["psi0"], c3["target"], c3["weights"]) as hc:
        J0, G0, _ = hc.eval(c3["pulsevals"])
        with _open(g, op, 0) as h:
            J, G, tau = h.eval(op["pulsevals"])
            print(dict(J=J, Gmax=np.abs(G).max(), timings=h.timings(), work=h.work()))
            assert np.isfinite(J) and np.all(np.isfinite(G)) and np.abs(G).max() > 0.0
            assert abs(J - (1.0 - abs(tau.sum()) ** 2 / 9.0)) <= 1e-14
            J1, G1, _ = hc.eval(c3["pulsevals"])
        J2, G2, _ = hc.eval(c3["pulsevals"])
    assert J1 == J0 and np.array_equal(G1, G0)
    assert J2 == J0 and np.array_equal(G2, G0)
