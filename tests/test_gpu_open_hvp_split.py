"""grape_open_hvp_forward / grape_open_hvp_backward / grape_open_hvp_backward_chi: split-phase Hessian-vector products on
open-system handles (csrc/grape_lindblad_hvp_split.hip.h) -- needs an MI355X.

The unsharded halves against grape_open_hvp bit for bit on every NP; two shards against the forward-over-forward reference of
tests/open_hvp_reference.py; the caller's route against tests/open_hvp_split_reference.py (proved by
tests/test_open_hvp_split_reference.py) with the Hilbert-Schmidt functional on every NP, and with chi = c sigma against
grape_open_hvp; bitwise independence of nv, order and repetition; non-interference; every refusal and the ordering rules;
GRAPE_ERR_TAYLOR.  N_T = 3, K <= 3, nv <= 5 throughout.

The comparison with a reference is open_hvp_split_reference.assert_open_hvp_split_agrees (caller's route) or
open_hvp_reference.assert_open_hvp_agrees (built-in route): ||d(Hv)||_inf <= 1e-10 max(||Hv||_inf, 1e-3) after conditions on the
reference alone.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_hvp_reference as ohr  # noqa: E402
import open_hvp_split_reference as osr  # noqa: E402
from open_hvp_reference import RE, SM, SS  # noqa: E402
from test_gpu_open_hvp import CASES as HVP_CASES, THETA, _kernel_beta, _open, _tlist  # noqa: E402

pytestmark = pytest.mark.gpu

GRID = dict(weights=True, shape=True, nonuniform=True)

# built-in route on two shards: the K = 3 case of tests/test_gpu_open_hvp.py (its reference is shared), and one at NP = 48
SHARD_CASES = dict(HVP_CASES, d48_J2_L1_K3_ss=dict(d=48, J=2, L=1, K=3, functional=SS, weights=True, nonuniform=True, nv=1))

# caller's route, Hilbert-Schmidt functional against sigma = the case's target (open_hvp_split_reference.reference_of); where
# the target of the pulse 0.8 x leaves the signals small the case takes the target of -0.8 x (tests/test_gpu_open_hvp.py)
CHI_CASES = {
    "d5": dict(d=5, J=2, L=2, K=2, functional=SM, nv=5, **GRID),
    "d16_L3_J8": dict(d=16, J=8, L=3, K=2, functional=SM, nonuniform=True, nv=2),
    "d17_K3_no_target": dict(d=17, J=2, L=2, K=3, functional=SM, no_target=True, nv=2, **GRID),
    "d33_non_hermitian": dict(d=33, J=1, L=2, K=2, functional=SM, hermitian=False, non_hermitian_states=0.3, nonuniform=True, nv=1),
    "d64_J8_no_target": dict(d=64, J=8, L=2, K=1, functional=SM, no_target=True, factor=-0.8, nonuniform=True, nv=1),
}


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


def _sums(h):
    return complex(*h.sums()[:2])


def _split(h, V):
    """both halves of the built-in route on an unsharded handle"""
    dtau, dsums = h.open_hvp_forward(V)
    return h.open_hvp_backward(_sums(h), dsums), dtau, dsums


def _hs_boundary(pr, sigma):
    return osr.hilbert_schmidt(sigma, pr.get("weights"))


def _hs_product(h, pr, sigma, V):
    """forward half, the Hilbert-Schmidt boundary formed on the host from rho(T) and rho'(T), backward half"""
    _, _, drho = h.open_hvp_forward(V, final_states=True)
    _, chi, dchi = _hs_boundary(pr, sigma)(h.final_states(), drho if drho.ndim == 4 else drho[None])
    return h.open_hvp_backward_chi(chi, dchi if drho.ndim == 4 else dchi[0]), drho


# ---- 1. the unsharded halves are grape_open_hvp, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d4_J2_L2_sm", "d17_J8_L3_K3_sm", "d32_J4_L2_ss", "d49_J5_L2_ss", "d63_J2_L2_re"])
def test_unsharded_halves_give_the_bits_of_open_hvp(g, name):
    pr, V, want = ohr.reference_of(name, HVP_CASES)
    x = pr["pulsevals"]
    K, L, nv = pr["H0"].shape[0], np.asarray(pr["Hc"]).shape[-3], len(V)
    with _open(g, pr) as h:
        h.eval(x)
        one = h.open_hvp(V)
        info_one = h.open_hvp_info()
        dtau, dsums, drho = h.open_hvp_forward(V, final_states=True)
        info_fw = h.open_hvp_info()
        two = h.open_hvp_backward(_sums(h), dsums)
        info = h.open_hvp_info()
    assert np.array_equal(one, two)
    assert info_fw["terms_forward"] == info_fw["series_terms"] == info_one["terms_forward"] and info_fw["terms_backward"] == 0
    assert info["terms_forward"] == info_one["terms_forward"] and info["terms_backward"] == info_one["terms_backward"]
    assert info["series_terms"] == info_one["series_terms"] and info["series_steps"] == info_one["series_steps"]
    assert info["dirs_per_group"] == nv and info["bytes"] > info_one["bytes"] and info["ms"] > 0.0
    w = np.ones(K) if pr.get("weights") is None else pr["weights"]
    fig = dict(dtau=float(np.abs(dtau - want["dtau"]).max()), dsums=float(np.abs(dsums - want["dtau"] @ w).max()),
               tau_of_drho=float(np.abs(osr.inner(pr["target"][None], drho) - want["dtau"]).max()))
    if pr["H0"].shape[1] <= 17:     # rho'(T) itself against the reference's (every NP: the tests of the caller's route)
        st = osr.stack_to_T(pr, x, V)
        fig["drho"] = float(np.abs(drho - st["drhoT"]).max())
        assert np.abs(st["drhoT"]).max() >= 1e-2
    print(name, fig)
    assert drho.shape == (nv, K, pr["H0"].shape[1], pr["H0"].shape[1])
    assert all(v <= 1e-12 for v in fig.values())
    ohr.assert_open_hvp_agrees(two, want, name)


# ---- 2. two shards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d17_J8_L3_K3_sm", "d48_J2_L1_K3_ss"])
def test_two_shards_against_the_reference_and_the_single_handle(g, name):
    """2 + 1 of K_total = 3 trajectories with weights: the host adds the partial sums between the halves and the partial
    products at the end, as ShardedEvaluator.hvp_host does"""
    pr, V, want = ohr.reference_of(name, SHARD_CASES)
    x = pr["pulsevals"]
    assert pr["H0"].shape[0] == 3 and pr["weights"] is not None
    with _open(g, pr) as h:
        h.eval(x)
        single = h.open_hvp(V)
    cut = lambda lo, hi: dict(pr, H0=pr["H0"][lo:hi], rho0=pr["rho0"][lo:hi], target=pr["target"][lo:hi], weights=pr["weights"][lo:hi])  # noqa: E731
    with _open(g, cut(0, 2), K_total=3) as h0, _open(g, cut(2, 3), K_total=3) as h1:
        shards = (h0, h1)
        for h in shards:
            h.forward(x)
        f_total = sum(_sums(h) for h in shards)
        fw = [h.open_hvp_forward(V) for h in shards]
        df_total = fw[0][1] + fw[1][1]
        got = sum(h.open_hvp_backward(f_total, df_total) for h in shards)
        dtau = np.concatenate([fw[0][0], fw[1][0]], axis=1)
        # the gradient's halves do not disturb the product's: a backward half of the gradient, then the product again
        for h in shards:
            h.backward(f_total)
        again = sum(h.open_hvp_backward(f_total, df_total) for h in shards)
    assert np.array_equal(got, again)
    assert np.abs(dtau - want["dtau"]).max() <= 1e-12 and np.abs(df_total - want["dtau"] @ pr["weights"]).max() <= 1e-12
    size = float(np.abs(single).max())
    print(name, dict(vs_single=float(np.abs(got - single).max()), size=size))
    assert np.abs(got - single).max() <= 1e-12 * size
    ohr.assert_open_hvp_agrees(got, want, name)


# ---- 3. the caller's route against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CHI_CASES))
def test_callers_route_with_the_hilbert_schmidt_functional(g, name):
    pr, V, sigma, want = osr.reference_of(name, CHI_CASES)
    x = pr["pulsevals"]
    K, L = pr["H0"].shape[0], np.asarray(pr["Hc"]).shape[-3]
    with _open(g, pr) as h:
        h.forward(x)
        dtau, dsums, drho = h.open_hvp_forward(V, final_states=True)
        rhoT = h.final_states()
        J, chi, dchi = _hs_boundary(pr, sigma)(rhoT, drho)
        got = h.open_hvp_backward_chi(chi, dchi)
        info = h.open_hvp_info()
        G = h.backward_chi(chi)
    fig = dict(J=abs(J - want["J"]), rho=float(np.abs(rhoT - want["rhoT"]).max()), drho=float(np.abs(drho - want["drhoT"]).max()),
               G=float(np.abs(G - want["G"]).max()))
    print(name, fig)
    assert fig["J"] <= 1e-12 and fig["rho"] <= 1e-12 and fig["drho"] <= 1e-12 and fig["G"] <= 1e-10 * max(np.abs(want["G"]).max(), 1e-3)
    if pr.get("target") is None:          # tau is NaN on such a handle, so are its derivatives
        assert np.all(np.isnan(dtau)) and np.all(np.isnan(dsums))
    else:
        assert np.abs(dtau - want["dtau"]).max() <= 1e-12
    assert info["series_steps"] >= len(V) * (K + K * L) * 3 and info["terms_backward"] > 0
    assert info["series_terms"] == info["terms_forward"] + info["terms_backward"]
    osr.assert_open_hvp_split_agrees(got, want, name)


def test_callers_route_at_d48_through_an_interval_of_three_substeps(g):
    """the case of tests/test_gpu_open_hvp.py::test_d48_one_interval_of_three_substeps: interval 1 is cut into three sub-steps, all
    four chains carry over; the count is asserted from the info call"""
    from grape_jl_amd import synth
    import open_helpers as oh
    d, L, K, N_T, nv = 48, 1, 1, 3, 2
    pr = synth.make_open_problem(d, L, N_T, K, 8, seed=4808)
    beta = _kernel_beta(pr, 0, 1)
    dt1, dt0 = 2.25 * THETA / beta, 0.3 * THETA / beta
    assert 2 < 0.95 * beta * dt1 / THETA and beta * dt1 / THETA < 3
    pr["tlist"] = _tlist([dt0, dt1, dt0])
    pr["functional"] = SS
    oh.order_one_states(pr, 4808, factor=-0.8)
    x = pr["pulsevals"]
    V = ohr.directions(4808, nv, x.size)
    sigma = pr["target"]
    want = osr.evaluate_chi(pr, x, V, _hs_boundary(pr, sigma))
    with _open(g, pr) as h:
        h.forward(x)
        got, drho = _hs_product(h, pr, sigma, V)
        info = h.open_hvp_info()
    assert np.abs(drho - want["drhoT"]).max() <= 1e-12
    osr.assert_open_hvp_split_agrees(got, want, "d48, three sub-steps")
    assert info["series_steps"] == nv * (K + K * L) * (1 + 3 + 1)


# ---- 4. the caller's route with the built-in boundary formed in numpy ------------------------------------------------------------
@pytest.mark.parametrize("functional", [SM, SS, RE])
def test_callers_route_with_c_sigma_is_open_hvp(g, functional):
    pr, V, _ = ohr.reference_of("d5_J2", HVP_CASES)
    x, w, sg, K = pr["pulsevals"], pr["weights"], pr["target"], 2
    with _open(g, pr, functional=functional) as h:
        _, _, tau = h.eval(x)
        want = h.open_hvp(V)
        dtau, dsums = h.open_hvp_forward(V)
        f = _sums(h)
        if functional == SM:
            c, dc = w * f / K ** 2, w[None] * dsums[:, None] / K ** 2
        elif functional == SS:
            c, dc = w * tau / K, w[None] * dtau / K
        else:
            c, dc = w / (2.0 * K) + 0j, np.zeros_like(dtau)
        got = h.open_hvp_backward_chi(c[:, None, None] * sg, dc[:, :, None, None] * sg[None])
        builtin = h.open_hvp_backward(f, dsums)
    size = float(np.abs(want).max())
    print(dict(functional=functional, dev=float(np.abs(got - want).max()), size=size))
    assert size >= 1e-3 and np.array_equal(builtin, want)
    assert np.abs(got - want).max() <= 1e-12 * size


# ---- 5. bitwise -------------------------------------------------------------------------------------------------------------------
def test_a_direction_does_not_depend_on_nv_order_or_repetition(g):
    pr, V, sigma, want = osr.reference_of("d5", CHI_CASES)
    x = pr["pulsevals"]
    assert len(V) == 5
    perm = np.array([3, 0, 4, 2, 1])
    with _open(g, pr) as h:
        h.eval(x)
        builtin, _, dsums = _split(h, V)
        chi_all, _ = _hs_product(h, pr, sigma, V)
        # two backward halves of either kind after ONE forward half
        _, _, drho = h.open_hvp_forward(V, final_states=True)
        _, chi, dchi = _hs_boundary(pr, sigma)(h.final_states(), drho)
        a = h.open_hvp_backward_chi(chi, dchi)
        b = h.open_hvp_backward(_sums(h), dsums)
        c = h.open_hvp_backward_chi(chi, dchi)
        d = h.open_hvp_backward(_sums(h), dsums)
        assert np.array_equal(a, chi_all) and np.array_equal(c, chi_all) and np.array_equal(b, builtin) and np.array_equal(d, builtin)
        singles = [(_split(h, v)[0], _hs_product(h, pr, sigma, v)[0]) for v in V]
        assert np.array_equal(np.stack([s[0] for s in singles]), builtin) and np.array_equal(np.stack([s[1] for s in singles]), chi_all)
        assert singles[0][0].shape == x.shape                       # a vector in, a vector out
        assert np.array_equal(_split(h, V[perm])[0], builtin[perm])
        assert np.array_equal(_hs_product(h, pr, sigma, V[perm])[0], chi_all[perm])
        assert np.array_equal(h.open_hvp(V), builtin)
    osr.assert_open_hvp_split_agrees(chi_all, want, "d5, five directions")


def test_the_split_calls_disturb_nothing(g):
    pr, V, sigma, _ = osr.reference_of("d5", CHI_CASES)
    x = pr["pulsevals"]
    X = np.stack([x, 0.5 * x])
    with _open(g, pr) as h:
        J, G, tau = h.eval(x)
        before = dict(dJdt=h.time_gradient(), hv=h.open_hvp(V), batch=h.open_eval_batch(X), tg=h.tau_grads(), work=h.work(), store=h.storage(0))
        bytes_before = h.open_hvp_info()["bytes"]
        _split(h, V)
        _hs_product(h, pr, sigma, V)
        assert np.array_equal(h.time_gradient(), before["dJdt"]) and np.array_equal(h.tau_grads(), before["tg"])
        assert h.work() == before["work"] and np.array_equal(h.storage(0), before["store"])
        batch = h.open_eval_batch(X)
        assert all(np.array_equal(p, q) for p, q in zip(batch, before["batch"]))
        assert np.array_equal(h.open_hvp(V), before["hv"])
        J1, G1, tau1 = h.eval(x)
        assert J1 == J and np.array_equal(G1, G) and np.array_equal(tau1, tau)
        assert np.array_equal(h.time_gradient(), before["dJdt"]) and np.array_equal(h.open_hvp(V), before["hv"])
    with _open(g, pr) as h:          # a handle that never makes a split call holds what it held before
        h.eval(x)
        h.open_hvp(V)
        assert h.open_hvp_info()["bytes"] == bytes_before


# ---- 6. refusals and ordering -----------------------------------------------------------------------------------------------------
def test_refusals_and_ordering_name_the_reason_and_leave_the_handle_usable(g, monkeypatch):
    from grape_jl_amd import synth
    pr, V, sigma, _ = osr.reference_of("d5", CHI_CASES)
    x = pr["pulsevals"]
    V2 = V[:2]
    zero = np.zeros((2, 2, 5, 5), complex)
    with _open(g, pr) as h:
        first = h.eval(x)

        def same_eval():
            J, G, tau = h.eval(x)
            assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(tau, first[2])

        def refused(needle, *more):
            for call, name in ((lambda: h.open_hvp_backward(1.0 + 0j, np.zeros(2, complex)), "grape_open_hvp_backward: "),
                               (lambda: h.open_hvp_backward_chi(zero[0], zero), "grape_open_hvp_backward_chi: ")):
                with pytest.raises(g.GrapeHipError) as err:
                    call()
                assert err.value.code == -1 and name in str(err.value) and needle in str(err.value), str(err.value)
                assert all(m in str(err.value) for m in more)

        refused("no grape_open_hvp_forward on this handle yet")
        same_eval()
        dtau, dsums = h.open_hvp_forward(V2)
        ok = h.open_hvp_backward(_sums(h), dsums)
        h.eval(x)
        refused("a forward evaluation came since")
        h.open_hvp_forward(V2)
        h.set_tlist(pr["tlist"])
        refused("grape_set_tlist came since")
        same_eval()
        h.open_hvp_forward(V2)
        h.eval_batch(np.stack([x, 0.5 * x]))
        refused("grape_eval_batch came since")
        same_eval()
        h.open_hvp_forward(V2)
        h.set_running_cost(None, 0.0)
        refused("grape_open_set_running_cost came since")
        same_eval()
        h.open_hvp_forward(V2)
        h.open_hvp(V2)
        refused("grape_open_hvp came since", "overwrites")
        same_eval()
        h.open_hvp_forward(V)                      # five directions
        refused("nv = 2", "took nv = 5")
        same_eval()
        # what does NOT invalidate a forward half: the batched evaluation, the time gradient, a backward half of the gradient
        h.open_hvp_forward(V2)
        h.open_eval_batch(np.stack([x, 0.5 * x]))
        h.time_gradient()
        h.backward(_sums(h))
        h.time_gradient()
        assert np.array_equal(h.open_hvp_backward(_sums(h), dsums), ok)
        # a cost set: every split call refuses, and says why
        D = np.diag(np.arange(5.0)).astype(complex)
        h.set_running_cost(D, 0.3)
        h.eval(x)
        for call in (lambda: h.open_hvp_forward(V2), lambda: h.open_hvp_backward(_sums(h), dsums), lambda: h.open_hvp_backward_chi(zero[0], zero)):
            with pytest.raises(g.GrapeHipError) as err:
                call()
            assert err.value.code == -1 and "running cost" in str(err.value) and "grape_open_hvp_" in str(err.value)
        h.set_running_cost(None, 0.0)
        same_eval()
        with pytest.raises(g.GrapeHipError) as err:      # the cost came and went: no forward half survives it
            h.open_hvp_backward(_sums(h), dsums)
        assert "came since" in str(err.value)
        h.open_hvp_forward(V2)
        assert np.array_equal(h.open_hvp_backward(_sums(h), dsums), ok)
        same_eval()
        h.check()
    # no forward state at all
    with _open(g, pr) as h:
        with pytest.raises(g.GrapeHipError) as err:
            h.open_hvp_forward(V2)
        assert err.value.code == -1 and "grape_open_hvp_forward: no valid forward state" in str(err.value)
        h.eval(x)
    # a handle without targets: the built-in half names the caller's route, which works
    with _open(g, dict(pr, target=None)) as hn:
        hn.forward(x)
        dtau, dsums, drho = hn.open_hvp_forward(V2, final_states=True)
        assert np.all(np.isnan(dtau)) and np.all(np.isnan(dsums)) and np.all(np.isfinite(drho))
        with pytest.raises(g.GrapeHipError) as err:
            hn.open_hvp_backward(1.0 + 0j, np.ones(2, complex))
        assert err.value.code == -1 and "no target states" in str(err.value) and "grape_open_hvp_backward_chi" in str(err.value)
        _, chi, dchi = _hs_boundary(pr, sigma)(hn.final_states(), drho)
        assert np.all(np.isfinite(hn.open_hvp_backward_chi(chi, dchi)))
    # a closed handle: the message names the closed calls
    cl = synth.make_problem(5, 2, 3, 2, seed=77)
    with g.GrapeHip(cl["H0"], cl["Hc"], cl["tlist"], cl["psi0"], cl["target"]) as hc:
        Jc, Gc, _ = hc.eval(cl["pulsevals"])
        v = np.ascontiguousarray(V[0])
        assert hc._lib.grape_open_hvp_forward(hc._h, 1, v.ctypes.data, None, None, None) == -1
        msg = hc._lib.grape_last_error(hc._h)
        assert b"not an open-system handle" in msg and b"grape_hvp_forward" in msg
        J2, G2, _ = hc.eval(cl["pulsevals"])
        assert J2 == Jc and np.array_equal(G2, Gc)
    # the inherited closed split calls stay the refusal they are on an open handle
    with _open(g, pr) as h:
        h.eval(x)
        with pytest.raises(g.GrapeHipError) as err:
            h.hvp_forward(V2)
        assert err.value.code == -1 and "open-system" in str(err.value)
        same = h.eval(x)
        assert same[0] == first[0] and np.array_equal(same[1], first[1])
    # more directions than stay resident (GRAPE_HVP_DIRS, read at create): the message carries the largest nv
    monkeypatch.setenv("GRAPE_HVP_DIRS", "2")
    with _open(g, pr) as h:
        h.eval(x)
        with pytest.raises(g.GrapeHipError) as err:
            h.open_hvp_forward(V)
        assert err.value.code == -1 and "nv = 5" in str(err.value) and "at most 2" in str(err.value)
        dtau, dsums = h.open_hvp_forward(V2)
        assert np.array_equal(h.open_hvp_backward(_sums(h), dsums), ok)
        J, G, tau = h.eval(x)
        assert J == first[0] and np.array_equal(G, first[1])
    monkeypatch.delenv("GRAPE_HVP_DIRS")


# ---- 7. a series that cannot converge ------------------------------------------------------------------------------------------------
def test_a_series_that_cannot_converge_is_grape_err_taylor(g):
    """The recipe of tests/test_gpu_open_hvp.py: input that is not finite (every norm is NaN, no stopping rule holds, the first
    series runs into the 200-term limit and every later one is cut after one term) -- here in chi', after a forward half on finite
    directions.  An error status, not a fault; the forward half stays valid and finite input gives the first result bit for bit."""
    pr, V, sigma, _ = osr.reference_of("d5", CHI_CASES)
    x = pr["pulsevals"]
    with _open(g, pr) as h:
        first = h.eval(x)
        _, _, drho = h.open_hvp_forward(V, final_states=True)
        _, chi, dchi = _hs_boundary(pr, sigma)(h.final_states(), drho)
        good = h.open_hvp_backward_chi(chi, dchi)
        bad = dchi.copy()
        bad[1, 0, 0, 0] = np.nan
        with pytest.raises(g.GrapeHipError) as err:
            h.open_hvp_backward_chi(chi, bad)
        assert err.value.code == -5 and "grape_open_hvp_backward_chi" in str(err.value) and "did not converge" in str(err.value)
        assert np.array_equal(h.open_hvp_backward_chi(chi, dchi), good)       # ... without a new forward half
        Vn = V.copy()
        Vn[1, 0] = np.nan
        with pytest.raises(g.GrapeHipError) as err:
            h.open_hvp_forward(Vn)
        assert err.value.code == -5 and "did not converge" in str(err.value)
        with pytest.raises(g.GrapeHipError) as err:                          # a failed forward half leaves nothing to read
            h.open_hvp_backward_chi(chi, dchi)
        assert err.value.code == -1 and "failed" in str(err.value)
        h.open_hvp_forward(V)
        assert np.array_equal(h.open_hvp_backward_chi(chi, dchi), good)
        J, G, tau = h.eval(x)
        assert J == first[0] and np.array_equal(G, first[1]) and np.array_equal(tau, first[2])
        h.check()
