"""The derivative kernels a small problem gets BY DEFAULT, against the absolute references -- needs an MI355X.

tests/conftest.py pins GRAPE_DERIV3=1 for the session, so that the one-wave assembly kernels -- the subject of most GPU tests --
are exercised by the suite's tiny problems.  A user has no such pin: with few derivative batches grape_create selects a
workgroup per batch (deriv_kernel<16>, deriv_kernel<32> for Hermitian N <= 32, deriv2_kernel with the economized series at
NP = 48, 64).  Every test here removes the pin with monkeypatch and keeps the bar of the test it repeats."""
import os

import numpy as np
import pytest

import test_gpu_parity as parity
import test_gpu_scan as scan

pytestmark = pytest.mark.gpu

TOL_J, TOL_TAU, tol_G = parity.TOL_J, parity.TOL_TAU, parity.tol_G


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    return mod


@pytest.fixture(autouse=True)
def default_route(monkeypatch):
    monkeypatch.delenv("GRAPE_DERIV3", raising=False)


# ---------------------------------------------------------------- what the suite runs pinned, once more without the pin

@pytest.mark.parametrize("path", parity.GOLDEN, ids=[os.path.basename(p) for p in parity.GOLDEN])
@pytest.mark.parametrize("method", [0, 1], ids=["gradgen", "taylor"])
def test_golden_fixtures_without_the_pin(g, path, method):
    """every golden fixture, the README problem (c1_readme_tls.npz) among them"""
    parity.test_golden_fixtures(g, path, method)


@pytest.mark.parametrize("prop", [0, 1], ids=["expprop", "series"])
@pytest.mark.parametrize("cid", ["C1", "C2"])
def test_baseline_configs_c1_c2_without_the_pin(g, ref, cid, prop):
    parity.test_baseline_configs_c1_c2_full_parity(g, ref, cid, prop)


_SCAN = scan.test_scan_against_the_sequential_sweeps_and_the_oracle
_SCAN_CASES = _SCAN.pytestmark[0].args[1]


@pytest.mark.parametrize("N,L,N_T,K,f,herm,bk", _SCAN_CASES)
def test_scan_against_the_sequential_sweeps_and_the_oracle_without_the_pin(g, ref, N, L, N_T, K, f, herm, bk):
    _SCAN(g, ref, N, L, N_T, K, f, herm, bk)


# ---------------------------------------------------------------- 50-digit pins

@pytest.mark.parametrize("name", ["herm64", "edge64"])
@pytest.mark.parametrize("functional", [0, 1, 2])
def test_absolute_pins_at_n64_on_the_workgroup_per_batch_kernel(g, name, functional):
    """N = 64, K = 2, few batches: expm_t16_asm, then deriv2_kernel with the economized series.  Bars of
    tests/test_gpu_reference_pins.py: 1e-13 of the scale, 2e-13 for G and tau_grads."""
    from conftest import load_mpmath_pin64
    pr, want = load_mpmath_pin64(name)
    w = want[functional]
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=functional) as h:
        J, G, tau, psiT = h.eval(pr["pulsevals"], want_psiT=True)
        tg, work = h.tau_grads(), h.work()
    assert int(work["asm_kernel"]) == 1 and int(work["asm_deriv_kernel"]) == 0, work
    sJ, sG, sT = max(1.0, abs(w["J"])), np.abs(w["G"]).max(), max(1.0, np.abs(w["tau"]).max())
    err = dict(J=abs(J - w["J"]) / sJ, tau=np.abs(tau - w["tau"]).max() / sT, G=np.abs(G - w["G"]).max() / sG,
               psiT=np.abs(psiT - w["psiT"]).max() / sT, tg=np.abs(tg - w["tau_grads"]).max() / np.abs(w["tau_grads"]).max())
    print(name, functional, {k: "%.2e" % v for k, v in err.items()}, "series orders", work["deriv_orders"])
    assert err["J"] <= 1e-13 and err["tau"] <= 1e-13 and err["psiT"] <= 1e-13
    assert err["G"] <= 2e-13 and err["tg"] <= 2e-13, err


@pytest.mark.parametrize("functional", [0, 1, 2])
def test_absolute_pin_at_n4_on_deriv_kernel_16(g, functional):
    """the Hermitian N = 4 pin (60 digits): deriv_kernel<16> behind the concurrent sweeps.  1e-13 of the scale."""
    from conftest import load_mpmath_pin
    pr, want = load_mpmath_pin("herm")
    w = want[functional]
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=functional) as h:
        J, G, tau, psiT = h.eval(pr["pulsevals"], want_psiT=True)
        tg, work = h.tau_grads(), h.work()
    assert int(work["asm_deriv_kernel"]) == 0
    sJ, sG, sT = max(1.0, abs(w["J"])), np.abs(w["G"]).max(), max(1.0, np.abs(w["tau"]).max())
    assert abs(J - w["J"]) <= 1e-13 * sJ and np.abs(tau - w["tau"]).max() <= 1e-13 * sT
    assert np.abs(G - w["G"]).max() <= 1e-13 * sG, np.abs(G - w["G"]).max() / sG
    assert np.abs(psiT - w["psiT"]).max() <= 1e-13 * sT
    assert np.abs(tg - w["tau_grads"]).max() <= 1e-13 * np.abs(w["tau_grads"]).max()


# ---------------------------------------------------------------- both sides of the `few` thresholds

def expected_few(NP, nbatch, num_cus):
    """grape_create, Hermitian NP < 48: a workgroup per batch when the batches are few"""
    if NP == 16:
        return nbatch <= 256
    return 0.14 * np.ceil(nbatch / num_cus) < 0.20 * np.ceil(nbatch / (4.0 * num_cus))


@pytest.mark.parametrize("N", [16, 32])
@pytest.mark.parametrize("N_T", [256, 257])
def test_both_sides_of_the_few_batches_threshold(g, ref, monkeypatch, N, N_T):
    """K = 16: 256 derivative batches at N_T = 256, 272 at 257.  grape_get_work[15] is 0 for both kernels below N = 49, so the
    route shows in the bits: the default's G is the GRAPE_DERIV3=0 run's below the threshold and the GRAPE_DERIV3=1 run's
    above it, and those two differ."""
    import torch
    from grape_jl_amd import synth
    K, L = 16, 2
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    few = bool(expected_few(N, K * ((N_T + 15) // 16), cus))
    if cus == 256:
        assert few == (N_T == 256)
    pr = synth.make_problem(N, L, N_T, K, seed=900 + N + N_T)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    res = {}
    for name, env in (("default", None), ("workgroup", "0"), ("wave", "1")):
        if env is not None:
            monkeypatch.setenv("GRAPE_DERIV3", env)
        with g.GrapeHip(*args) as h:
            res[name] = h.eval(pr["pulsevals"])
        monkeypatch.delenv("GRAPE_DERIV3", raising=False)
    differ = not np.array_equal(res["workgroup"][1], res["wave"][1])
    print(dict(N=N, N_T=N_T, cus=cus, few=few, kernels_differ=differ,
               dG=float(np.abs(res["workgroup"][1] - res["wave"][1]).max())))
    assert differ, "the two kernels give the same bits for this seed: the case proves nothing"
    assert np.array_equal(res["default"][1], res["workgroup" if few else "wave"][1])
    assert res["default"][0] == res["workgroup"][0] == res["wave"][0]
    Jr, Gr, taur = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], gradient_method=ref.TAYLOR)
    for J, G, tau in res.values():
        assert abs(J - Jr) <= TOL_J and np.abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr)


# ---------------------------------------------------------------- features on the default route at NP = 48, 64

def _nonuniform(N_T, seed):
    from grape_jl_amd import synth
    return np.concatenate([[0.0], np.cumsum(0.5 + 0.5 * synth.uniform01(seed, N_T))])


@pytest.mark.parametrize("N", [48, 64])
@pytest.mark.parametrize("kind", ["shape-nonuniform-pertraj", "general-drift"])
def test_features_on_deriv2_kernel_with_the_economized_series(g, N, kind):
    """K = 2, N_T = 21 (a partial last batch): shaped amplitudes, a non-uniform grid and control operators per trajectory
    together; and a general drift beside Hermitian controls.  Against oracle/grape_oracle.py, which knows shapes."""
    import grape_oracle as go
    from grape_jl_amd import synth
    L, N_T, K = 2, 21, 2
    herm = kind != "general-drift"
    pr = synth.make_problem(N, L, N_T, K, seed=7300 + N, hermitian=herm)
    tl = _nonuniform(N_T, seed=N)
    w = np.array([0.7, 1.3])
    Hc, shape = pr["Hc"], None
    if herm:
        Hc = np.stack([np.stack([synth.gue(synth.subseed(7300 + N, 500 + 10 * k + l), N) for l in range(L)]) for k in range(K)])
        shape = 0.5 + np.abs(np.sin(np.arange(float(L * N_T)))).reshape(L, N_T)
    with g.GrapeHip(pr["H0"], Hc, tl, pr["psi0"], pr["target"], w, shape=shape) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        work = h.work()
    assert int(work["asm_deriv_kernel"]) == 0, work
    if herm and N == 64:
        assert int(work["asm_kernel"]) == 3, work          # expm_t16p_asm
    Jr, Gr, taur = go.evaluate_gradient(pr["H0"], Hc, tl, pr["pulsevals"], pr["psi0"], pr["target"], w, shape=shape)
    sc = max(1.0, np.abs(taur).max()) ** 2
    print(dict(N=N, kind=kind, dJ=abs(J - Jr), dtau=float(np.abs(tau - taur).max()), dG=float(np.abs(G - Gr).max()),
               G_max=float(np.abs(Gr).max()), series_orders=work["deriv_orders"]))
    assert abs(J - Jr) <= TOL_J * sc and np.abs(tau - taur).max() <= TOL_TAU * sc and np.abs(G - Gr).max() <= tol_G(Gr)
