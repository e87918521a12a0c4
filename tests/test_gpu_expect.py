"""grape_expect (csrc/grape_expect.hip.h): observables on the stored forward states, on the device -- needs an MI355X.

The reference is tests/expect_reference.py (proved in tests/test_expect_reference.py): ``numpy.einsum`` on ``h.storage(0)`` of
the same handle with the derived rounding bound of ``assert_expect_agrees`` (closed: 2 . 4 (N + 4) u ||O||_F ||psi||^2, open:
2 . 2 (d^2 + 4) u ||O||_F ||rho||_F, u = 2^-53), and independent propagations (frame_reference, open_reference) at the project's
TOL_SCALAR = 1e-12.  N_T is 3, 16 or 33: 4, 17 and 34 grid points -- a partial block of 16, a full block plus one, two full
blocks plus two.  Operators have unit 2-norm and O(1) expectation values on normalised states; every set carries one
non-Hermitian operator, and every case asserts on the reference alone that each observable reaches max_n |e| >= 0.05.
"""
import numpy as np
import pytest

import expect_reference as er
import frame_reference as fr
import grape_jl_amd as g
import open_reference as orf
from grape_jl_amd import synth

pytestmark = pytest.mark.gpu

EXP, SER = g.PROP_EXP, g.PROP_SERIES
SM, SS, RE = 0, 1, 2
_CACHE = {}


def closed_problem(N, K, N_T, kind="herm", seed=None):
    """a well-scaled twin of frame_reference.make_twin: built once, shared, never modified"""
    key = ("closed", N, K, N_T, kind, seed)
    if key not in _CACHE:
        _CACHE[key] = fr.make_twin(N, 2, K, N_T, seed=(6000 + 10 * N + N_T) if seed is None else seed, kind=kind)
    return _CACHE[key]


def handle(p, functional=SM, prop=EXP, **kw):
    return g.GrapeHip(p["H0"], p["Hc"], p["tlist"], p["psi0"], p["target"], p["weights"], functional=functional,
                      shape=p["shape"], prop_method=prop, **kw)


def open_problem(d, K=2, N_T=3, J=2, seed=None):
    key = ("open", d, K, N_T, J, seed)
    if key not in _CACHE:
        seed_ = (7000 + 10 * d + N_T) if seed is None else seed
        pr = synth.make_open_problem(d, 2, N_T, K, J, seed=seed_)
        v = synth.unit_vectors(synth.subseed(seed_, 8000), K, d)
        pr["rho0"] = v[:, :, None] * v[:, None, :].conj()            # unit Frobenius norm
        u = synth.uniform01(synth.subseed(seed_, 8100), N_T)
        pr["tlist"] = np.concatenate([[0.0], np.cumsum(0.5 + u)])
        _CACHE[key] = pr
    return _CACHE[key]


def open_handle(pr, functional=SM, **kw):
    return g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr["target"], pr["weights"],
                          functional=functional, **kw)


def ops_for(N, M, seed, K=None):
    """M operators (per trajectory with K), the non-Hermitian one at position 1 (position 0 when it is alone)"""
    return er.observables(N, M, seed, K, non_hermitian=(0,) if M == 1 else (1,))


def check_closed(h, ops, label):
    fw = h.storage(0)
    want = er.expect_closed(fw, ops)
    er.assert_order_one(want)
    got = h.expect(ops)
    er.assert_expect_agrees(got, want, ops, fw, label)
    return got


def check_open(h, ops, label):
    store = h.storage(0)
    want = er.expect_open(store, ops)
    er.assert_order_one(want)
    got = h.expect(ops)
    er.assert_expect_agrees(got, want, ops, store, label)
    return got


# ---- against einsum on storage(0) of the same handle ------------------------------------------------------------------------
CLOSED = {
    "N5_K1_M1_T3": dict(N=5, K=1, M=1, N_T=3),
    "N16_K3_M16_T16": dict(N=16, K=3, M=16, N_T=16),
    "N17_K3_M3_T33_pertraj": dict(N=17, K=3, M=3, N_T=33, per_traj=True),
    "N48_K1_M3_T16_pertraj": dict(N=48, K=1, M=3, N_T=16, per_traj=True),
    "N64_K3_M16_T33": dict(N=64, K=3, M=16, N_T=33),
    "N64_K1_M1_T3": dict(N=64, K=1, M=1, N_T=3),
    "N20_general_K3_M3_T3": dict(N=20, K=3, M=3, N_T=3, kind="general"),
    "N20_general_K1_M16_T16_pertraj": dict(N=20, K=1, M=16, N_T=16, kind="general", per_traj=True),
    "N100_blocked_K1_M3_T3": dict(N=100, K=1, M=3, N_T=3),
    "N100_blocked_K3_M1_T16_pertraj": dict(N=100, K=3, M=1, N_T=16, per_traj=True),
    "N20_series_K3_M3_T16": dict(N=20, K=3, M=3, N_T=16, prop=SER),
    "N20_series_K1_M16_T33_pertraj": dict(N=20, K=1, M=16, N_T=33, prop=SER, per_traj=True),
}


@pytest.mark.parametrize("name", list(CLOSED))
def test_closed_against_einsum_on_the_stored_states(name):
    c = CLOSED[name]
    pr = closed_problem(c["N"], c["K"], c["N_T"], c.get("kind", "herm"))
    ops = ops_for(c["N"], c["M"], 100 + c["N"], c["K"] if c.get("per_traj") else None)
    with handle(pr, prop=c.get("prop", EXP)) as h:
        h.eval(pr["pulsevals"])
        got = check_closed(h, ops, name)
        info = h.expect_info()
    assert got.shape == (c["K"], c["N_T"] + 1, c["M"])
    NP = 16 * ((c["N"] + 15) // 16) if c["N"] <= 64 else (128 if c["N"] <= 128 else 256)
    assert info["M"] == c["M"] and info["bytes"] > 0 and info["ms"] > 0.0
    assert info["mfma_flop"] >= 8.0 * c["N"] ** 2 * c["K"] * (c["N_T"] + 1) * c["M"]     # (padding and block granularity add to it)
    assert info["mfma_flop"] == c["K"] * ((c["N_T"] + 16) // 16) * c["M"] * (NP // 16) * (NP // 4) * 4 * 2048.0


OPEN = {
    "d3_T3": dict(d=3, N_T=3), "d16_T16": dict(d=16, N_T=16), "d17_T33_pertraj": dict(d=17, N_T=33, per_traj=True),
    "d33_T16": dict(d=33, N_T=16), "d64_T3": dict(d=64, N_T=3),
}


@pytest.mark.parametrize("name", list(OPEN))
def test_open_against_einsum_on_the_stored_states(name):
    c = OPEN[name]
    pr = open_problem(c["d"], N_T=c["N_T"])
    ops = ops_for(c["d"], 3, 200 + c["d"], 2 if c.get("per_traj") else None)
    with open_handle(pr) as h:
        h.forward(pr["pulsevals"])
        got = check_open(h, ops, name)
        info = h.expect_info()
    assert got.shape == (2, c["N_T"] + 1, 3)
    assert info["M"] == 3 and info["bytes"] > 0 and info["mfma_flop"] == 0.0


# ---- against an independent propagation at TOL_SCALAR ------------------------------------------------------------------------
@pytest.mark.parametrize("N,N_T", [(17, 16), (64, 3)])
def test_closed_against_an_independent_propagation(N, N_T):
    pr = closed_problem(N, 2, N_T)
    ops = ops_for(N, 3, 300 + N)
    want = er.expect_closed(fr.propagate(pr, pr["pulsevals"], derivatives=False)["fw"], ops)
    er.assert_order_one(want)
    with handle(pr) as h:
        h.forward(pr["pulsevals"])
        got = h.expect(ops)
    dev = float(np.abs(got - want).max())
    print(f"N = {N}: max deviation {dev:.2e}")
    assert dev <= fr.TOL_SCALAR


def test_skewed_twin_in_the_balanced_frame_gives_the_twins_values():
    """e[0] = -3, e[-1] = +3: the handle balances, stores D^-1 Psi and uploads D O D; the caller's O_s = S^-1 O S^-1"""
    N, N_T = 17, 16
    pr = closed_problem(N, 2, N_T, "general")
    e = fr.skew_exponents(N, 4117)
    ops = ops_for(N, 3, 317, K=2)
    want = er.expect_closed(fr.propagate(pr, pr["pulsevals"], derivatives=False)["fw"], ops)
    er.assert_order_one(want)
    ps, ops_s = fr.skewed(pr, e), er.skewed_ops(ops, e)
    with handle(ps) as h:
        h.eval(pr["pulsevals"])
        got = h.expect(ops_s)
        check_closed(h, ops_s, "skewed, einsum on storage(0) in the caller's frame")
    dev = float(np.abs(got - want).max())
    print(f"skewed twin: max deviation {dev:.2e}")
    assert dev <= fr.TOL_SCALAR
    assert np.abs(er.expect_closed(fr.propagate(ps, pr["pulsevals"], derivatives=False)["fw"], er.skewed_ops(ops, e, wrong="similarity"))
                  - want).max() > 1e-3     # (the mistake the frame rule excludes is visible on this problem)


@pytest.mark.parametrize("d", [17, 33])
def test_open_against_an_independent_propagation(d):
    pr = open_problem(d, N_T=3)
    ops = ops_for(d, 3, 400 + d, K=2)
    L, N_T = 2, 3
    x = np.asarray(pr["pulsevals"]).reshape(L, N_T)
    states = [np.asarray(pr["rho0"], complex)]
    for n in range(1, N_T + 1):     # rho(t_n): the reference's final state on the first n intervals
        states.append(orf.propagate(pr, x[:, :n].reshape(-1), tlist=pr["tlist"][:n + 1], gradient=False)["rhoT"])
    want = er.expect_open(np.stack(states, axis=1), ops)
    er.assert_order_one(want)
    with open_handle(pr) as h:
        h.forward(pr["pulsevals"])
        got = h.expect(ops)
    dev = float(np.abs(got - want).max())
    print(f"d = {d}: max deviation {dev:.2e}")
    assert dev <= fr.TOL_SCALAR


# ---- cross-checks with device paths that already exist -------------------------------------------------------------------
def test_closed_running_cost_is_the_trapezoid_sum_of_expect():
    N, N_T = 33, 16
    pr = closed_problem(N, 3, N_T)
    D = fr.penalty(N, 77)
    with handle(pr, D=D, lambda_b=0.3) as h:
        h.eval(pr["pulsevals"])
        e = h.expect(D[None])
        jb = h.sums()[4]
    mine = float(np.sum(fr.trapezoid_weights(pr["tlist"])[None, :] * e[:, :, 0].real))
    print(dict(sums4=jb, trapezoid=mine))
    assert jb >= 1e-2 and abs(mine - jb) <= 1e-12


def test_open_running_cost_is_the_trapezoid_sum_of_expect():
    d, N_T = 17, 16
    pr = open_problem(d, N_T=N_T)
    D = np.stack([fr.penalty(d, 78), fr.penalty(d, 79)])
    with open_handle(pr) as h:
        h.set_running_cost(D, 0.25)
        h.eval(pr["pulsevals"])
        e = h.expect(D[:, None])
        jb = h.sums()[4]
        check_open(h, ops_for(d, 3, 417), "open handle with a running cost")
    mine = float(np.sum(fr.trapezoid_weights(pr["tlist"])[None, :] * e[:, :, 0].real))
    print(dict(sums4=jb, trapezoid=mine))
    assert jb >= 1e-2 and abs(mine - jb) <= 1e-12


# ---- handle state ---------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def test_expect_between_graph_replays_leaves_every_evaluation_its_bits():
    pr = closed_problem(48, 2, 16)
    ops = ops_for(48, 3, 548)
    x = pr["pulsevals"]
    with handle(pr) as h:
        first = h.eval(x)
        for _ in range(4):                      # (the third evaluation onwards replays the captured graph)
            assert _same(h.eval(x), first)
        for rnd in range(4):
            check_closed(h, ops, f"between replays, round {rnd}")
            assert _same(h.eval(x), first)
        check_closed(h, ops, "after the last evaluation")
        # another pulse in between: the stored states, and with them the values, move
        e0 = h.expect(ops)
        h.eval(0.5 * x)
        e1 = check_closed(h, ops, "other pulse")
        assert np.abs(e1 - e0).max() > 1e-3
        assert _same(h.eval(x), first)


def test_derivative_getters_answer_with_the_same_bits_after_expect():
    pr = closed_problem(20, 2, 16)
    ops = ops_for(20, 16, 520)
    x = pr["pulsevals"]
    V = np.stack([np.cos(np.arange(x.size)), np.sin(np.arange(x.size))])
    with handle(pr) as h:
        h.eval(x)
        before = (h.time_gradient(), h.hvp(V), h.tau_grads(), h.storage(0), h.work()["cells"])
        a = check_closed(h, ops, "N = 20, M = 16")
        after = (h.time_gradient(), h.hvp(V), h.tau_grads(), h.storage(0), h.work()["cells"])
        assert _same(before, after)
        assert np.array_equal(h.expect(ops), a)
    pr = open_problem(17, N_T=16)
    ops = ops_for(17, 3, 517)
    x = pr["pulsevals"]
    V = np.stack([np.cos(np.arange(x.size)), np.sin(np.arange(x.size))])
    with open_handle(pr) as h:
        first = h.eval(x)
        before = (h.time_gradient(), h.open_hvp(V), h.tau_grads(), h.storage(0))
        a = check_open(h, ops, "d = 17")
        after = (h.time_gradient(), h.open_hvp(V), h.tau_grads(), h.storage(0))
        assert _same(before, after)
        assert np.array_equal(h.expect(ops), a)
        h.open_eval_batch(np.stack([x, 0.5 * x]))          # (does not invalidate the store)
        assert np.array_equal(h.expect(ops), a)
        assert _same(h.eval(x), first)


@pytest.mark.parametrize("N,N_T", [(17, 33), (64, 16), (100, 3)])
def test_an_observable_has_the_same_bits_alone_and_inside_a_set(N, N_T):
    pr = closed_problem(N, 2, N_T)
    ops = ops_for(N, 16, 600 + N)
    with handle(pr) as h:
        h.forward(pr["pulsevals"])
        full = h.expect(ops)
        assert np.array_equal(h.expect(ops), full)
        for m in (0, 15, 1):
            assert np.array_equal(h.expect(ops[m][None])[..., 0], full[..., m]), m
        rev = h.expect(ops[::-1])
        assert np.array_equal(rev[..., ::-1], full)
        assert h.expect_info()["M"] == 16


def test_an_open_observable_has_the_same_bits_alone_and_inside_a_set():
    pr = open_problem(33, N_T=16)
    ops = ops_for(33, 16, 633)
    with open_handle(pr) as h:
        h.forward(pr["pulsevals"])
        full = h.expect(ops)
        assert np.array_equal(h.expect(ops), full)
        for m in (0, 15):
            assert np.array_equal(h.expect(ops[m][None])[..., 0], full[..., m]), m
        assert np.array_equal(h.expect(ops[::-1])[..., ::-1], full)


# ---- shards -----------------------------------------------------------------------------------------------------------------
def test_two_shards_behind_one_handle_with_operators_per_trajectory():
    pr = closed_problem(17, 3, 16)
    ops = ops_for(17, 3, 717, K=3)
    with handle(pr, devices=[0, 0]) as h:
        h.eval(pr["pulsevals"])
        got = check_closed(h, ops, "devices = [0, 0]")
        info = h.expect_info()
        assert info["M"] == 3 and info["bytes"] > 0 and info["mfma_flop"] > 0
    with handle(pr) as h1:                      # the same numbers as one device, bit for bit (trajectories are independent)
        h1.eval(pr["pulsevals"])
        assert np.array_equal(h1.expect(ops), got)


def test_split_phase_shard():
    pr = closed_problem(20, 4, 16)
    ops = ops_for(20, 3, 720, K=4)
    x = pr["pulsevals"]
    with handle(pr) as h:
        h.forward(x)
        whole = h.expect(ops)
    for lo in (0, 2):
        sl = slice(lo, lo + 2)
        with g.GrapeHip(pr["H0"][sl], pr["Hc"], pr["tlist"], pr["psi0"][sl], pr["target"][sl], pr["weights"][sl], shape=pr["shape"],
                        K_total=4) as h:
            h.forward(x)
            got = check_closed(h, ops[sl], f"shard [{lo}, {lo + 2})")
        assert got.shape == (2, 17, 3) and np.array_equal(got, whole[sl])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _refused(h, ops, text):
    with pytest.raises(g.GrapeHipError) as ei:
        h.expect(ops)
    assert ei.value.code == -1 and "grape_expect: " in str(ei.value) and text in str(ei.value), str(ei.value)


def test_refusals_leave_the_handle_as_it_was():
    pr = closed_problem(17, 2, 16)
    ops = ops_for(17, 3, 817)
    x = pr["pulsevals"]
    with handle(pr) as h:
        _refused(h, ops, "no evaluation on this handle yet")
        first = h.eval(x)
        a = check_closed(h, ops, "first")
        bytes0 = h.expect_info()["bytes"]
        h.expect(ops)
        info = h.expect_info()
        assert info["M"] == 3 and info["bytes"] == bytes0 and info["mfma_flop"] > 0      # (the same size: nothing grows)
        _refused(h, er.observables(17, 17, 1), "16")
        assert _same(h.eval(x), first)
        h.eval_batch(np.stack([x, 0.5 * x]))
        _refused(h, ops, "grape_eval_batch")
        assert _same(h.eval(x), first)
        assert np.array_equal(h.expect(ops), a)
        h.set_tlist(pr["tlist"])
        _refused(h, ops, "grape_set_tlist")
        assert _same(h.eval(x), first)                 # (the same grid: the same bits)
        assert np.array_equal(h.expect(ops), a)
        assert h.expect_info()["bytes"] == bytes0
        big = h.expect(ops_for(17, 16, 818))           # more observables: the buffers grow, the values of the others do not move
        assert big.shape == (2, 17, 16) and h.expect_info()["bytes"] > bytes0
        assert np.array_equal(h.expect(ops), a)


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one-device", "two-shards"])
def test_refused_after_a_failed_evaluation(devices):
    """weights = [0, 1] under J_T_ss: chi_0(T) = 0, the evaluation with a gradient raises GRAPE_ERR_CHI_NORM"""
    pr = dict(closed_problem(17, 2, 16), weights=np.array([0.0, 1.0]))
    ops = ops_for(17, 3, 819)
    x = pr["pulsevals"]
    with handle(pr, functional=SS, devices=devices) as h:
        first = h.eval(x, gradient=False)
        a = check_closed(h, ops, "functional only")
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval(x)
        assert ei.value.code == -3
        _refused(h, ops, "the last evaluation failed")
        again = h.eval(x, gradient=False)
        assert first[0] == again[0] and np.array_equal(first[2], again[2])
        assert np.array_equal(h.expect(ops), a)


def test_open_refusals():
    pr = open_problem(17, N_T=16)
    ops = ops_for(17, 3, 917)
    x = pr["pulsevals"]
    with open_handle(pr) as h:
        _refused(h, ops, "no evaluation on this handle yet")
        first = h.eval(x)
        a = check_open(h, ops, "first")
        _refused(h, er.observables(17, 17, 2), "16")
        h.set_tlist(pr["tlist"])
        _refused(h, ops, "grape_set_tlist")
        assert _same(h.eval(x), first)
        h.set_running_cost(fr.penalty(17, 80), 0.5)
        _refused(h, ops, "grape_open_set_running_cost")
        h.set_running_cost(None, 0.0)
        _refused(h, ops, "grape_open_set_running_cost")
        assert _same(h.eval(x), first)             # (after removal: the bits of a handle that never had a cost)
        assert np.array_equal(h.expect(ops), a)
        h.eval_batch(np.stack([x, 0.5 * x]))
        _refused(h, ops, "grape_eval_batch")
        assert _same(h.eval(x), first)


def test_open_refused_after_a_failed_evaluation():
    """weights = [0, 1] under J_T_ss on an open handle: the backward half raises GRAPE_ERR_CHI_NORM"""
    pr = dict(open_problem(17, N_T=16), weights=np.array([0.0, 1.0]))
    ops = ops_for(17, 3, 919)
    x = pr["pulsevals"]
    with open_handle(pr, functional=SS) as h:
        first = h.eval(x, gradient=False)
        a = check_open(h, ops, "functional only")
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval(x)
        assert ei.value.code == -3
        _refused(h, ops, "the last evaluation failed")
        again = h.eval(x, gradient=False)
        assert first[0] == again[0] and np.array_equal(first[2], again[2])
        assert np.array_equal(h.expect(ops), a)
        h.forward(x)
        assert np.array_equal(h.expect(ops), a)
