"""grape_hvp_forward / grape_hvp_backward / grape_hvp_backward_chi on the GPU: the Hessian-vector product of grape_hvp cut
at its one cross-trajectory dependency (include/grape_hip.h, csrc/grape_hvp_split.hip.h).

Bars: against the references (tests/hvp_reference.py, tests/hvp_split_reference.py, both proved on the CPU) the project's
gradient tolerance applied to H v, ||dHv||_inf <= 1e-10 max(||Hv||_inf, 1e-3) (``hr.assert_hvp_agrees``), with ||G||_inf and
||Hv||_inf >= 1e-3 asserted on the reference alone; between two routes of the library 1e-12 ||Hv||_inf (the bar of
test_route_independence_at_n64); tau'_k and Psi'_k(T) within 1e-12 max(1, ||.||_inf), the project's tau bound; and
``np.array_equal`` wherever the same kernels run on the same data.  Every case has N_T = 4 and K <= 3.
"""
import numpy as np
import pytest

import grape_jl_amd as g
import hvp_reference as hr
import hvp_split_reference as sr
import test_gpu_hvp as base
from grape_jl_amd import synth

pytestmark = pytest.mark.gpu

N_T = base.N_T
_cache = {}


def handle(pr, functional, sl=None, target=True, **kw):
    """a handle of the whole problem, or of the trajectories ``sl`` as a shard of it (K_total = K of the problem)"""
    sl = slice(None) if sl is None else sl
    Hc = pr["Hc"][sl] if np.ndim(pr["Hc"]) == 4 else pr["Hc"]
    return g.GrapeHip(pr["H0"][sl], Hc, pr["tlist"], pr["psi0"][sl], pr["target"][sl] if target else None, pr["weights"][sl],
                      functional=functional, shape=pr["shape"], K_total=pr["K"], **kw)


def f_of(sums):
    return complex(sums[0], sums[1])


def builtin_reference(name):
    """tau', Psi'(T) of a case of tests/test_gpu_hvp.py (its H v reference is shared with that file)"""
    if ("builtin", name) not in _cache:
        pr, f, V, want = base.case(name)
        _cache[("builtin", name)] = sr.evaluate_chi(pr, pr["pulsevals"], V, sr.builtin_boundary(pr, f))
    return _cache[("builtin", name)]


@pytest.mark.parametrize("name", ["N3-L1-sm", "N16-L8-ss", "N16-L2-re", "N33-L2-sm-general-skewed", "N17-L8-sm-K2-shape",
                                  "N64-L8-re-pertraj"])
def test_unsharded_halves_give_the_bits_of_hvp(name):
    pr, f, V, want = base.case(name)
    ref = builtin_reference(name)
    with handle(pr, f) as h:
        h.eval(pr["pulsevals"])
        whole = h.hvp(V)
        info_whole = h.hvp_info()
        dtau, dsums, dpsiT = h.hvp_forward(V, final_states=True)
        info_fw = h.hvp_info()
        halves = h.hvp_backward(f_of(h.sums()), dsums)
        info_bw = h.hvp_info()
    hr.assert_hvp_agrees(whole, want["Hv"], name)
    base.assert_second_tile_agrees(halves, want["Hv"], pr["L"], name)
    assert np.array_equal(whole, halves)
    for tag, got, exp in (("dtau", dtau, ref["dtau"]), ("dpsiT", dpsiT, ref["dpsiT"]),
                          ("dsums", dsums, (ref["dtau"] * pr["weights"][None, :]).sum(axis=1))):
        dev, bound = float(np.abs(got - exp).max()), 1e-12 * max(1.0, float(np.abs(exp).max()))
        print(name, tag, dict(dev=dev, bound=bound, max=float(np.abs(exp).max())))
        assert got.shape == exp.shape and dev <= bound, (tag, dev, bound)
    print(info_whole, info_fw, info_bw)
    assert info_fw["series_terms"] == info_fw["terms_forward"] == info_whole["terms_forward"] and info_fw["terms_backward"] == 0
    assert info_bw["terms_forward"] == info_fw["terms_forward"] and info_bw["terms_backward"] == info_whole["terms_backward"]
    assert info_bw["series_terms"] == info_whole["series_terms"] and info_bw["series_steps"] == info_whole["series_steps"]
    assert info_fw["series_steps"] == pr["K"] * len(V) * N_T and info_bw["ms"] > 0


SHARDED = {
    "N17-sm-herm": dict(N=17, L=2, K=3, f=0, weights=True),
    "N33-ss-general-skewed": dict(N=33, L=2, K=3, f=1, herm=False, skew=3, weights=True),
}


def sharded_case(name):
    if ("sharded", name) not in _cache:
        c = dict(SHARDED[name])
        f = c.pop("f")
        pr = base.make_case(seed=2000 + sum(map(ord, name)), **c)
        V = hr.directions(sum(map(ord, name)), 2, pr["L"] * N_T)
        _cache[("sharded", name)] = (pr, f, V, hr.evaluate(pr, pr["pulsevals"], V, f))
    return _cache[("sharded", name)]


@pytest.mark.parametrize("name", list(SHARDED))
def test_two_shards_on_one_gpu(name):
    """K = 3 as 2 + 1 with K_total = 3 and weights: dsums, f and the partial H v are added in numpy"""
    pr, f, V, want = sharded_case(name)
    hr.assert_order_one(want)
    x = pr["pulsevals"]
    with handle(pr, f) as h:
        h.eval(x)
        single = h.hvp(V)
    with handle(pr, f, slice(0, 2)) as a, handle(pr, f, slice(2, 3)) as b:
        a.forward(x), b.forward(x)
        f_total = f_of(a.sums()) + f_of(b.sums())
        (_, dsa), (_, dsb) = a.hvp_forward(V), b.hvp_forward(V)
        Hv = a.hvp_backward(f_total, dsa + dsb) + b.hvp_backward(f_total, dsa + dsb)
    hr.assert_hvp_agrees(Hv, want["Hv"], name)
    rel = float(np.abs(Hv - single).max() / np.abs(single).max())
    print(name, dict(shards_vs_single_rel=rel))
    assert rel <= 1e-12


CHI = {
    "N3-L1": dict(N=3, L=1, K=2),
    "N16-L8": dict(N=16, L=8, K=2, amp=1.0),
    "N17-L3-K3-weights-shape-nonuniform-no-targets": dict(N=17, L=3, K=3, weights=True, shape=True, nonuniform=True, target=False),
    "N33-L2-general-skewed": dict(N=33, L=2, K=2, herm=False, skew=3),
    # two column tiles on three waves: hvp_backward_chi_kernel<48, 2>
    "N33-L8": dict(N=33, L=8, K=2, amp=1.0),
    "N48-L1-K1-long-interval": dict(N=48, L=1, K=1, dt=4.0),
    "N64-L2-no-targets": dict(N=64, L=2, K=2, nv=1, target=False),
}


def chi_case(name):
    """(problem, has targets, directions, boundary of the expectation-value functional, reference)"""
    if ("chi", name) not in _cache:
        c = dict(CHI[name])
        nv, target = c.pop("nv", 2), c.pop("target", True)
        seed = 3000 + sum(map(ord, name))
        pr = base.make_case(seed=seed, **c)
        V = hr.directions(sum(map(ord, name)), nv, pr["L"] * N_T)
        boundary = sr.expectation_boundary(sr.observables(seed, pr["K"], pr["N"]), pr["weights"])
        want = sr.evaluate_chi(pr if target else dict(pr, target=None), pr["pulsevals"], V, boundary)
        _cache[("chi", name)] = (pr, target, V, boundary, want)
    return _cache[("chi", name)]


def caller_route(h, x, V, boundary):
    """what a caller with a functional of their own does: forward, Psi(T), Psi'(T), their chi and chi', backward halves"""
    h.forward(x)
    psiT = h.final_states()
    dtau, dsums, dpsiT = h.hvp_forward(V, final_states=True)
    both = [boundary(psiT, d) for d in dpsiT]
    chi, dchi = both[0][1], np.stack([b[2] for b in both])
    return dict(J=both[0][0], G=h.backward_chi(chi), Hv=h.hvp_backward_chi(chi, dchi), dtau=dtau, dsums=dsums, dpsiT=dpsiT, psiT=psiT)


@pytest.mark.parametrize("name", list(CHI))
def test_callers_functional_against_the_reference(name):
    pr, target, V, boundary, want = chi_case(name)
    sr.assert_signals(want)
    with handle(pr, 0, target=target) as h:
        got = caller_route(h, pr["pulsevals"], V, boundary)
        info = h.hvp_info()
    assert abs(got["J"] - want["J"]) <= 1e-12 and np.abs(got["G"] - want["G"]).max() <= hr.tol_hv(want["G"])
    hr.assert_hvp_agrees(got["Hv"], want["Hv"], name)
    base.assert_second_tile_agrees(got["Hv"], want["Hv"], pr["L"], name)
    dev, bound = float(np.abs(got["dpsiT"] - want["dpsiT"]).max()), 1e-12 * max(1.0, float(np.abs(want["dpsiT"]).max()))
    print(name, dict(dpsiT_dev=dev, bound=bound), info)
    assert dev <= bound
    if target:
        assert np.abs(got["dtau"] - want["dtau"]).max() <= 1e-12 * max(1.0, float(np.abs(want["dtau"]).max()))
    else:   # tau is NaN on a handle without targets, and so are its derivatives
        assert np.isnan(got["dtau"]).all() and np.isnan(got["dsums"]).all()
    steps = 2 * pr["K"] * len(V) * N_T
    if name == "N48-L1-K1-long-interval":   # every interval is cut at least once (see tests/test_gpu_hvp.py)
        assert info["series_steps"] >= 2 * steps, info
        assert info["series_steps"] % (2 * len(V)) == 0
    else:
        assert info["series_steps"] == steps, info
    assert info["series_terms"] == info["terms_forward"] + info["terms_backward"] and info["terms_backward"] > 0


def test_callers_functional_on_two_shards():
    """the skewed general case as 1 + 1: every shard balances its own problem, chi and chi' are formed from the states of both"""
    name = "N33-L2-general-skewed"
    pr, _, V, boundary, want = chi_case(name)
    x = pr["pulsevals"]
    with handle(pr, 0, slice(0, 1)) as a, handle(pr, 0, slice(1, 2)) as b:
        a.forward(x), b.forward(x)
        psiT = np.concatenate([a.final_states(), b.final_states()])
        dpsiT = np.concatenate([a.hvp_forward(V, final_states=True)[2], b.hvp_forward(V, final_states=True)[2]], axis=1)
        both = [boundary(psiT, d) for d in dpsiT]
        chi, dchi = both[0][1], np.stack([q[2] for q in both])
        Hv = a.hvp_backward_chi(chi[0:1], dchi[:, 0:1]) + b.hvp_backward_chi(chi[1:2], dchi[:, 1:2])
    hr.assert_hvp_agrees(Hv, want["Hv"], name + " as two shards")


@pytest.mark.parametrize("functional", [0, 1, 2])
def test_callers_route_with_the_builtin_boundary_matches_hvp(functional):
    """chi = c_k tgt_k, chi' = c'_k tgt_k formed in numpy from tau and tau'"""
    pr, _, V, _ = base.case("N16-L2-re")
    w, K = pr["weights"], pr["K"]
    with handle(pr, functional) as h:
        _, _, tau = h.eval(pr["pulsevals"])
        whole = h.hvp(V)
        dtau, _ = h.hvp_forward(V)
        c = hr._coefficients(functional, tau, dtau[0], w, K)[0]
        dc = np.stack([hr._coefficients(functional, tau, d, w, K)[1] for d in dtau])
        Hv = h.hvp_backward_chi(c[:, None] * pr["target"], dc[:, :, None] * pr["target"][None])
    rel = float(np.abs(Hv - whole).max() / np.abs(whole).max())
    print(dict(functional=functional, rel=rel, Hv_max=float(np.abs(whole).max())))
    assert np.abs(whole).max() >= 1e-3 and rel <= 1e-12


def test_directions_do_not_see_each_other():
    """nv = 5 equals five calls and a permuted pair, bit for bit, on both routes; two backward halves after one forward half
    give the same bits"""
    pr, f, _, _ = base.case("N33-L2-sm-general-skewed")
    boundary = sr.expectation_boundary(sr.observables(77, pr["K"], pr["N"]), pr["weights"])
    V = hr.directions(77, 5, pr["L"] * N_T)
    x = pr["pulsevals"]

    def both_routes(h, W):
        psiT = h.final_states()
        dtau, dsums, dpsiT = h.hvp_forward(W, final_states=True)
        if W.ndim == 1:
            _, chi, dchi = boundary(psiT, dpsiT)
        else:
            q = [boundary(psiT, d) for d in dpsiT]
            chi, dchi = q[0][1], np.stack([r[2] for r in q])
        built_in = h.hvp_backward(f_of(h.sums()), dsums)
        callers = h.hvp_backward_chi(chi, dchi)
        assert np.array_equal(h.hvp_backward(f_of(h.sums()), dsums), built_in)      # a third and a fourth half
        assert np.array_equal(h.hvp_backward_chi(chi, dchi), callers)
        return built_in, callers, dtau, dpsiT

    with handle(pr, f) as h:
        h.forward(x)
        all5 = both_routes(h, V)
        again = both_routes(h, V)
        single = [both_routes(h, v) for v in V]
        pair = both_routes(h, V[[3, 1]])
    for i in range(4):
        assert np.array_equal(all5[i], again[i])
        assert np.array_equal(all5[i], np.stack([s[i] for s in single]))
        assert np.array_equal(pair[i], all5[i][[3, 1]])


def test_no_side_effect_on_the_evaluation_and_on_hvp():
    pr, f, V, _ = base.case("N16-L2-re")
    boundary = sr.expectation_boundary(sr.observables(5, pr["K"], pr["N"]), pr["weights"])
    K, L, NP, LN = pr["K"], pr["L"], 16, pr["L"] * N_T
    with handle(pr, f) as h:
        for _ in range(4):        # (beyond the second evaluation the captured graph replays)
            J0, G0, tau0 = h.eval(pr["pulsevals"])
        dJdt0, Hv0 = h.time_gradient(), h.hvp(V)
        # a handle that has made no split call holds what grape_hvp has always allocated for two directions: per direction
        # V, H v, K workspaces of 4 NP^2, Psi' [K][N_T+1][NP], tau', c', the terms [K][L N_T], 4 K statistics words; one flag word
        per = 2 * LN * 8 + K * (4 * NP * NP * 8 + (N_T + 1) * NP * 16 + 16 + 16 + LN * 16 + 4 * 8)
        assert h.hvp_info()["bytes"] == 2 * per + 8
        _, dsums, dpsiT = h.hvp_forward(V, final_states=True)
        h.hvp_backward(f_of(h.sums()), dsums)
        q = [boundary(pr["target"], d) for d in dpsiT]   # (any chi will do here: the targets stand in for Psi(T))
        h.hvp_backward_chi(q[0][1], np.stack([r[2] for r in q]))
        # the extras live in a store of their own: chi~ [K][NP], chi~' [nv][K][NP], zero targets [K][N], Psi'(T) packed for the
        # host [nv][K][N], f, f', partial sums
        assert h.hvp_info()["bytes"] == 2 * per + 8 + (K * NP + 2 * K * NP + K * pr["N"] + 2 * K * pr["N"]) * 16 + (2 + 2 * 2 + 2 * 2) * 8
        assert np.array_equal(h.time_gradient(), dJdt0)
        assert np.array_equal(h.hvp(V), Hv0)
        for _ in range(3):
            J1, G1, tau1 = h.eval(pr["pulsevals"])
            assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(tau1, tau0)
            _, dsums = h.hvp_forward(V[0])
            h.hvp_backward(f_of(h.sums()), dsums)
        assert np.array_equal(h.hvp(V), Hv0)


def _refused(call, what):
    with pytest.raises(g.GrapeHipError) as ei:
        call()
    assert ei.value.code == -1, ei.value
    assert "grape_hvp_" in str(ei.value) and what in str(ei.value), str(ei.value)


def test_state_and_refusals_leave_the_handle_usable(monkeypatch):
    pr, f, V, _ = base.case("N16-L2-re")
    x = pr["pulsevals"]
    chi, dchi = np.ones((pr["K"], 16), complex), np.ones((2, pr["K"], 16), complex)
    with handle(pr, f) as h:
        _refused(lambda: h.hvp_forward(V), "no valid forward state")             # nothing evaluated yet
        J0, G0, tau0 = h.eval(x)

        def same_bits():
            J1, G1, tau1 = h.eval(x)
            assert J1 == J0 and np.array_equal(G1, G0) and np.array_equal(tau1, tau0)

        f_total = f_of(h.sums())
        _refused(lambda: h.hvp_backward(f_total, np.zeros(2, complex)), "no grape_hvp_forward")   # backward before forward
        _refused(lambda: h.hvp_backward_chi(chi, dchi), "no grape_hvp_forward")
        same_bits()
        _, dsums = h.hvp_forward(V)
        first = h.hvp_backward(f_total, dsums)
        _refused(lambda: h.hvp_backward(f_total, dsums[:1]), "nv = 1")           # nv mismatch
        _refused(lambda: h.hvp_backward_chi(chi, dchi[0]), "nv = 1")
        assert np.array_equal(h.hvp_backward(f_total, dsums), first)             # ... and the forward half is still good
        same_bits()                                                              # an evaluation between the halves
        _refused(lambda: h.hvp_backward(f_total, dsums), "forward evaluation")
        _refused(lambda: h.hvp_backward_chi(chi, dchi), "forward evaluation")
        h.hvp_forward(V)
        h.set_tlist(pr["tlist"] * 1.25)
        _refused(lambda: h.hvp_backward(f_total, dsums), "grape_set_tlist")
        _refused(lambda: h.hvp_forward(V), "no valid forward state")
        h.set_tlist(pr["tlist"])
        same_bits()
        h.hvp_forward(V)
        h.eval_batch(np.stack([x, 0.9 * x]))
        _refused(lambda: h.hvp_backward(f_total, dsums), "grape_eval_batch")
        same_bits()
        h.hvp_forward(V)
        h.hvp(V)
        _refused(lambda: h.hvp_backward(f_total, dsums), "grape_hvp came")
        h.hvp_forward(V)
        assert np.array_equal(h.hvp_backward(f_total, dsums), first)
        same_bits()
    # launch groups limited to two directions: three cannot stay resident
    monkeypatch.setenv("GRAPE_HVP_DIRS", "2")
    with handle(pr, f) as h:
        J0, G0, _ = h.eval(x)
        _refused(lambda: h.hvp_forward(hr.directions(3, 3, pr["L"] * N_T)), "at most 2")
        _, dsums = h.hvp_forward(V)
        h.hvp_backward(f_of(h.sums()), dsums)
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
    monkeypatch.delenv("GRAPE_HVP_DIRS")
    # no targets: the built-in functional has no boundary
    with handle(pr, f, target=False) as h:
        tau0 = h.forward(x)
        _, dsums = h.hvp_forward(V)
        _refused(lambda: h.hvp_backward(0j, np.zeros(2, complex)), "no target states")
        assert np.array_equal(h.forward(x), tau0, equal_nan=True)
    # the built-in running cost
    D = np.diag(np.arange(16.0)).astype(complex)
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=f, D=D, lambda_b=0.1) as h:
        J0, G0, _ = h.eval(x)
        _refused(lambda: h.hvp_forward(V), "running cost")
        J1, G1, _ = h.eval(x)
        assert J1 == J0 and np.array_equal(G1, G0)
    # N = 65
    big = synth.make_problem(65, 1, N_T, 1, seed=5)
    with g.GrapeHip(big["H0"], big["Hc"], big["tlist"], big["psi0"], big["target"], big["weights"]) as h:
        J0, G0, _ = h.eval(big["pulsevals"])
        _refused(lambda: h.hvp_forward(np.ones(N_T)), "N > 64")
        _refused(lambda: h.hvp_backward_chi(np.ones((1, 65), complex), np.ones((1, 65), complex)), "N > 64")
        J1, G1, _ = h.eval(big["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)
    # an open-system handle
    op = synth.make_open_problem(4, 1, N_T, 1, 1, seed=5)
    with g.GrapeHipOpen(op["H0"], op["Hc"], op["cops"], op["tlist"], op["rho0"], op["target"]) as h:
        J0, G0, _ = h.eval(op["pulsevals"])
        _refused(lambda: h.hvp_forward(np.ones(N_T)), "open-system")
        _refused(lambda: h.hvp_backward(0j, np.zeros(1, complex)), "open-system")
        J1, G1, _ = h.eval(op["pulsevals"])
        assert J1 == J0 and np.array_equal(G1, G0)
