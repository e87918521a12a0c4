"""Parity of the HIP path (through the C ABI) against the oracle -- needs an MI355X.

Stated tolerance, GPU vs CPU restatement on identical inputs:
    |dJ| <= 1e-12,   |dtau_k| <= 1e-12,   ||dG||_inf <= 1e-10 * max(||G||_inf, 1e-3)
(the reference's own bar between its two gradient routes is 1e-10, test_tls_optimization.jl:229).
"""
import glob
import os

import numpy as np
import pytest
from scipy.linalg import expm

pytestmark = pytest.mark.gpu

TOL_J = 1e-12
TOL_TAU = 1e-12


def tol_G(Gref):
    return 1e-10 * max(np.abs(Gref).max(), 1e-3)


GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


def hip_eval(g, pr, functional=0, method=0, **kw):
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr.get("weights"),
                    functional=functional, gradient_method=method, **kw) as h:
        J, G, tau, psiT = h.eval(pr["pulsevals"], want_psiT=True)
        return J, G, tau, psiT, h.tau_grads()


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
@pytest.mark.parametrize("method", [0, 1], ids=["gradgen", "taylor"])
def test_golden_fixtures(g, path, method):
    z = np.load(path)
    pr = {k: z[k] for k in ("H0", "Hc", "tlist", "pulsevals", "psi0", "target", "weights")}
    J, G, tau, psiT, tg = hip_eval(g, pr, int(z["functional"]), method)
    assert abs(J - z["J"]) <= TOL_J
    assert np.abs(tau - z["tau"]).max() <= TOL_TAU
    assert np.abs(G - z["G"]).max() <= tol_G(z["G"])
    assert np.abs(psiT - z["psiT"]).max() <= 1e-12
    assert np.abs(tg - z["tau_grads"]).max() <= 1e-12


# which hand-written kernels a fixture must reach (grape_get_work[14..16]: exponential cell, derivative kernel, blocked products)
REACHES = {"n64_l2_k2_sm_herm.npz": dict(asm_kernel=1, asm_deriv_kernel=1),          # expm_t16_asm, deriv3_asm
           "n64_l2_k2_re_nonherm.npz": dict(asm_kernel=2, asm_deriv_kernel=3),       # expm_t18g_asm, deriv3g_asm
           "n64_l2_k3_sm_pertraj.npz": dict(asm_kernel=3),                           # expm_t16p_asm
           "n100_l2_k2_ss.npz": dict(asm_blocked_products=1, asm_deriv_kernel=4)}    # lg_gemm_asm, deriv4_asm_128


@pytest.mark.parametrize("name", sorted(REACHES))
def test_golden_fixtures_reach_the_assembly_kernels(g, name):
    """the round-6 fixtures exist to pin the HEADLINE kernels (every older fixture has N <= 20 and runs compiled kernels only):
    each of them must take the hand-written kernel it was made for -- and agree with the fixture's numbers, which
    julia/make_reference_fixtures.jl would replace by GRAPE.jl's own the day someone runs it"""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", name))
    pr = {k: z[k] for k in ("H0", "Hc", "tlist", "pulsevals", "psi0", "target", "weights")}
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"],
                    functional=int(z["functional"])) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        w = h.work()
        tg = h.tau_grads()
    for key, want in REACHES[name].items():
        assert int(w[key]) == want, (key, w[key], want)
    if REACHES[name].get("asm_kernel") in (1, 3):
        assert w["t16_cells"] == w["t18_cells"] > 0        # every cell took the four-product assembly route
    assert abs(J - z["J"]) <= TOL_J and np.abs(tau - z["tau"]).max() <= TOL_TAU
    assert np.abs(G - z["G"]).max() <= tol_G(z["G"])
    assert np.abs(tg - z["tau_grads"]).max() <= 1e-12


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_reference_outputs_when_present_gpu(g, path):
    """the HIP path against outputs of GRAPE.jl itself (tests/golden/ref_<name>.json, julia/make_reference_fixtures.jl);
    skipped while nobody with a Julia installation has produced them -- see tests/test_oracle.py"""
    from conftest import load_reference_outputs
    want = load_reference_outputs(path)
    if want is None:
        pytest.skip("no reference outputs committed (julia/make_reference_fixtures.jl has not been run)")
    z = np.load(path)
    pr = {k: z[k] for k in ("H0", "Hc", "tlist", "pulsevals", "psi0", "target", "weights")}
    for method, name in ((0, "gradgen"), (1, "taylor")):
        w = want[name]
        J, G, tau, psiT, tg = hip_eval(g, pr, int(z["functional"]), method)
        assert abs(J - w["J"]) <= TOL_J and np.abs(tau - w["tau"]).max() <= TOL_TAU
        assert np.abs(G - w["G"]).max() <= tol_G(w["G"])
        assert np.abs(psiT - w["psiT"]).max() <= 1e-12 and np.abs(tg - w["tau_grads"]).max() <= 1e-12


CASES = [  # N, L, N_T, K, dt, hermitian, functional
    (2, 1, 40, 1, 0.01, True, 0),     # Pade order 3
    (3, 2, 9, 2, 0.2, False, 1),      # order 5/7, ragged N
    (16, 1, 25, 4, 1.0, True, 0),     # C2-like, order 9
    (17, 2, 6, 2, 1.0, False, 2),     # pads to 32
    (32, 4, 5, 3, 1.0, True, 0),      # L = 4
    (33, 1, 4, 2, 1.0, True, 1),      # pads to 64 (48-wide tile config unused)
    (48, 2, 4, 2, 1.0, True, 0),
    (64, 2, 8, 3, 1.0, True, 0),      # C3-like, order 13, s = 0
    (64, 2, 4, 2, 4.0, True, 1),      # s = 2
    (64, 3, 4, 2, 9.0, False, 2),     # s = 3..4, non-Hermitian
    (64, 6, 3, 1, 1.0, True, 0),      # L = 6 (two-qubit-gate-like control count)
    (64, 2, 5, 2, 0.3, True, 2),      # Hermitian, low orders (9/7): the symmetric fast path falls back per cell
    (100, 2, 4, 2, 2.5, True, 0),     # blocked path, Hermitian upper-triangle products, s >= 1
]


@pytest.mark.parametrize("case", CASES, ids=[f"N{c[0]}_L{c[1]}_dt{c[4]}_{'h' if c[5] else 'nh'}_f{c[6]}" for c in CASES])
def test_random_problems_vs_c_oracle(g, ref, case):
    from grape_jl_amd import synth
    N, L, N_T, K, dt, herm, f = case
    pr = synth.make_problem(N, L, N_T, K, seed=1000 + N + L, dt=dt, hermitian=herm)
    pr["weights"] = 0.5 + np.arange(K) * 0.25
    J, G, tau, psiT, tg = hip_eval(g, pr, f, 0)
    Jr, Gr, taur, parts = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"],
                                       pr["weights"], functional=f, gradient_method=ref.GRADGEN, want_parts=True)
    assert abs(J - Jr) <= TOL_J
    assert np.abs(tau - taur).max() <= TOL_TAU
    assert np.abs(G - Gr).max() <= tol_G(Gr)
    assert np.abs(psiT - parts["psiT"]).max() <= 1e-12
    assert np.abs(tg - parts["tau_grads"]).max() <= 1e-10 * max(np.abs(parts["tau_grads"]).max(), 1e-3)


LARGE = [  # blocked path (64 < N <= 256): N, L, N_T, K, dt, hermitian, functional
    (65, 1, 3, 2, 1.0, True, 0),
    (100, 2, 4, 2, 1.0, False, 1),
    (128, 2, 3, 2, 3.0, True, 2),
    (200, 3, 3, 1, 1.0, True, 0),
    (256, 4, 3, 2, 1.0, True, 0),     # C5-like
]


@pytest.mark.parametrize("case", LARGE, ids=[f"N{c[0]}_L{c[1]}_dt{c[4]}_{'h' if c[5] else 'nh'}_f{c[6]}" for c in LARGE])
def test_blocked_path_vs_c_oracle(g, ref, case):
    """N > 64 runs the blocked (batched block-GEMM) variant; the oracle's :taylor route is the checker
    (the literal (L+1)N block exponential is too slow at these sizes; both oracle routes are pinned
    against each other in tests/test_oracle.py)."""
    from grape_jl_amd import synth
    N, L, N_T, K, dt, herm, f = case
    pr = synth.make_problem(N, L, N_T, K, seed=2000 + N, dt=dt, hermitian=herm)
    J, G, tau, psiT, tg = hip_eval(g, pr, f, 0)
    Jr, Gr, taur, parts = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"],
                                       pr["weights"], functional=f, gradient_method=ref.TAYLOR, want_parts=True)
    assert abs(J - Jr) <= TOL_J
    assert np.abs(tau - taur).max() <= TOL_TAU
    assert np.abs(G - Gr).max() <= tol_G(Gr)
    assert np.abs(psiT - parts["psiT"]).max() <= 1e-12


@pytest.mark.parametrize("herm", [True, False], ids=["herm", "general"])
def test_blocked_path_chunks_of_two_cells(g, ref, herm, monkeypatch):
    """The blocked path goes through the cells in chunks with one set of scratch.  Chunks of two cells here; the time grid
    makes the cells need 0, 1 and 2 squarings, so that early chunks go straight to U and later ones through the squaring
    launches.  Bit for bit the result of the default chunking (no floating-point sum crosses a chunk), and the oracle's."""
    from grape_jl_amd import synth
    N, L, N_T, K = 100, 2, 7, 2
    pr = synth.make_problem(N, L, N_T, K, seed=4100, dt=1.0, hermitian=herm)
    dts = np.array([0.6, 0.6, 2.4, 0.6, 4.9, 0.6, 0.6]) * (1.0 if herm else 0.4)
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(dts)])
    out = {}
    for chunk in ("2", None):
        if chunk:
            monkeypatch.setenv("GRAPE_LG_CHUNK", chunk)
        else:
            monkeypatch.delenv("GRAPE_LG_CHUNK", raising=False)
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], weights=pr["weights"]) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            J2, G2, tau2 = h.eval(pr["pulsevals"])          # (a second evaluation: the flags are cleared per evaluation)
            assert J == J2 and np.array_equal(G, G2)
            w = h.work()
            out[chunk] = (J, G.copy(), tau.copy(), h.propagator(1, 4), w["t18_squarings"])
    assert out["2"][0] == out[None][0] and np.array_equal(out["2"][1], out[None][1]) and np.array_equal(out["2"][2], out[None][2])
    assert np.array_equal(out["2"][3], out[None][3])
    assert out["2"][4] == out[None][4] and out["2"][4] > 0          # squarings happened, the same number
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                functional=0, gradient_method=ref.TAYLOR)[:3]
    assert abs(out["2"][0] - Jr) <= TOL_J and np.abs(out["2"][1] - Gr).max() <= tol_G(Gr)


def test_expm_kernel_vs_scipy(g):
    """The ExpProp step itself (optimize.jl:732): U_kn = exp(-i H_kn dt_n), every Pade branch."""
    from grape_jl_amd import synth
    for N, dt in [(16, 0.002), (16, 0.05), (32, 0.3), (64, 0.45), (64, 1.0), (64, 3.0), (64, 25.0), (96, 1.0),
                  (256, 0.02), (256, 1.0), (256, 6.0)]:
        pr = synth.make_problem(N, 2, 3, 2, seed=77, dt=dt)
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"]) as h:
            h.eval(pr["pulsevals"], gradient=False)
            for k, n in [(0, 0), (1, 2)]:
                eps = pr["pulsevals"].reshape(2, 3)[:, n]
                H = pr["H0"][k] + eps[0] * pr["Hc"][0] + eps[1] * pr["Hc"][1]
                R = expm(-1j * H * dt)
                U = h.propagator(k, n)
                assert np.abs(U - R).max() <= 2e-14 * max(1.0, dt), (N, dt)
                assert np.abs(U.conj().T @ U - np.eye(N)).max() <= 1e-13 * max(1.0, dt)


def test_shaped_amplitude_and_per_trajectory_controls(g):
    import grape_oracle as go
    from grape_jl_amd import synth
    pr = synth.make_problem(8, 2, 6, 3, seed=5)
    shape = 0.5 + np.abs(np.sin(np.arange(12.0))).reshape(2, 6)
    Hck = np.stack([pr["Hc"] * (1.0 + 0.1 * k) for k in range(3)])  # [K, L, N, N]
    with g.GrapeHip(pr["H0"], Hck, pr["tlist"], pr["psi0"], pr["target"], shape=shape) as h:
        J, G, tau = h.eval(pr["pulsevals"])
    Jr, Gr, taur = go.evaluate_gradient(pr["H0"], Hck, pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"],
                                        shape=shape)
    assert abs(J - Jr) <= TOL_J and np.abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr)


def test_functional_only_and_repeatability(g):
    from grape_jl_amd import synth
    pr = synth.make_problem(64, 2, 10, 4, seed=9)
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"]) as h:
        J0, G0, tau0 = h.eval(pr["pulsevals"], gradient=False)
        assert G0 is None
        J1, G1, tau1 = h.eval(pr["pulsevals"])
        J2, G2, tau2 = h.eval(pr["pulsevals"])
        assert J0 == J1 == J2 and np.array_equal(G1, G2) and np.array_equal(tau1, tau2)  # bitwise reproducible


def test_error_behaviour(g):
    # chi norm guard (optimize.jl:1021-1025): tau = 0 for J_T_sm
    H0 = np.zeros((1, 2, 2), complex)
    Hc = np.zeros((1, 2, 2), complex)
    with g.GrapeHip(H0, Hc, np.array([0., 1.]), np.array([[1, 0]], complex), np.array([[0, 1]], complex)) as h:
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval(np.array([0.3]))
        assert ei.value.code == -3 and "chi" in str(ei.value)
        J, _, tau = h.eval(np.array([0.3]), gradient=False)  # functional alone is fine
        assert abs(J - 1.0) < 1e-15
    # taylor non-convergence is an error, not a silent truncation (optimize.jl:644-648)
    from grape_jl_amd import synth
    pr = synth.make_problem(8, 1, 3, 1, seed=2, dt=6.0)
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], gradient_method=1,
                    taylor_max_order=4) as h:
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval(pr["pulsevals"])
        assert ei.value.code == -5
    # the size envelope is refused loudly, not emulated: materialised propagators up to N = 256, the matrix-free propagator
    # up to N = 512, at most eight controls
    pr = synth.make_problem(257, 1, 2, 1, seed=1)
    with pytest.raises(g.GrapeHipError) as ei:
        g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"])
    assert "GRAPE_PROP_SERIES" in str(ei.value)
    pr = synth.make_problem(513, 1, 2, 1, seed=1)
    with pytest.raises(g.GrapeHipError):
        g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], prop_method=g.PROP_SERIES)
    pr = synth.make_problem(20, 9, 2, 1, seed=1)
    with pytest.raises(g.GrapeHipError):
        g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"])


def test_split_phase_shards_equal_single_handle(g):
    """Sum over trajectories is the only coupling (optimize.jl:579): two K/2 shards with the
    all-reduced f reproduce the one-handle result (this is what the RCCL path does per rank)."""
    from grape_jl_amd import synth
    pr = synth.make_problem(32, 2, 12, 6, seed=21)
    J, G, tau, _, _ = hip_eval(g, pr)
    Gs, taus = [], []
    hs = [g.GrapeHip(pr["H0"][s], pr["Hc"], pr["tlist"], pr["psi0"][s], pr["target"][s], pr["weights"][s], K_total=6)
          for s in (slice(0, 2), slice(2, 6))]
    for h in hs:
        taus.append(h.forward(pr["pulsevals"]))
    f = sum(t.sum() for t in taus)
    for h in hs:
        Gs.append(h.backward(f))
        h.close()
    assert np.abs(np.concatenate(taus) - tau).max() <= 1e-14
    assert np.abs(Gs[0] + Gs[1] - G).max() <= 1e-15
    assert abs(1 - abs(f) ** 2 / 36 - J) <= 1e-15


@pytest.mark.parametrize("prop", [0, 1], ids=["expprop", "series"])
def test_headline_size_properties(g, prop):
    """Full C3 size (N=64, L=2, N_T=1000, K=128): size-independent properties --
    (i) central finite differences of the GPU functional, (ii) norm conservation of the stored
    states (Hermitian H), (iii) shard additivity of the gradient, (iv) J from tau -- for the ExpProp path
    and for the matrix-free propagator, and (v) both paths agree with each other."""
    from grape_jl_amd import synth
    pr = synth.make_config("C3")
    if prop == 1:
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"]) as h:
            Je, Ge, taue = h.eval(pr["pulsevals"])
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], prop_method=prop) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        if prop == 1:
            assert abs(J - Je) <= TOL_J and np.abs(tau - taue).max() <= TOL_TAU and np.abs(G - Ge).max() <= tol_G(Ge)
        assert abs(J - (1 - abs(tau.sum()) ** 2 / 128**2)) <= 1e-14
        fw = h.storage(0)
        assert np.abs(np.linalg.norm(fw, axis=2) - 1.0).max() <= 1e-11
        bw = h.storage(1)
        assert np.abs(np.linalg.norm(bw, axis=2) - 1.0).max() <= 1e-11
        eps = 1e-5
        for idx in (0, 777, 1000 + 333, 1999):
            xp, xm = pr["pulsevals"].copy(), pr["pulsevals"].copy()
            xp[idx] += eps
            xm[idx] -= eps
            fd = (h.eval(xp, gradient=False)[0] - h.eval(xm, gradient=False)[0]) / (2 * eps)
            assert abs(fd - G[idx]) <= 5e-10 + 1e-5 * abs(G[idx])
    # shard additivity at full size
    hs = [g.GrapeHip(pr["H0"][s], pr["Hc"], pr["tlist"], pr["psi0"][s], pr["target"][s], pr["weights"][s], K_total=128,
                     prop_method=prop)
          for s in (slice(0, 64), slice(64, 128))]
    taus = [h.forward(pr["pulsevals"]) for h in hs]
    f = sum(t.sum() for t in taus)
    Gs = [h.backward(f) for h in hs]
    for h in hs:
        h.close()
    assert np.abs(Gs[0] + Gs[1] - G).max() <= 1e-12 * max(np.abs(G).max(), 1e-3)


def test_device_pointer_api_matches_host_api(g):
    """grape_forward_device / grape_backward_device on torch-owned device buffers (what bench.py and the
    RCCL path use) give bitwise the same result as grape_eval."""
    import torch
    from grape_jl_amd import synth
    from grape_jl_amd.sharded import ShardedEvaluator
    pr = synth.make_problem(64, 2, 12, 3, seed=77)
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"]) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        dev = torch.device("cuda", 0)
        ev = ShardedEvaluator(h, 3, g.J_T_SM, dist=None, device=dev)
        x, out, Gd = ev.alloc_device(2, 12, 3)
        x.copy_(torch.from_numpy(pr["pulsevals"]))
        stream = torch.cuda.current_stream(dev).cuda_stream
        ev.eval_device(stream)
        h.check(stream)
        assert ev.J_device() == J
        assert np.array_equal(Gd.cpu().numpy(), G)
        assert np.array_equal(out[:6].cpu().numpy().view(np.complex128), tau)
        tm = h.timings()
        assert tm["expm"] > 0 and tm["deriv"] > 0
        w = h.work()
        assert w["cells"] == 36 and w["flop_expm"] > 0


def test_pivoted_fallback_for_unsafe_pade_denominators(g, ref, monkeypatch):
    """Cells whose Pade denominator q(A) defeats unpivoted elimination (a pi-pulse in ONE time step makes
    its diagonal vanish) are re-solved with partial pivoting (LAPACK gesv semantics of the reference)."""
    sx = np.array([[0, 1], [1, 0]], complex)
    sz = np.array([[1, 0], [0, -1]], complex)
    H0 = 1e-3 * sz[None]
    Hc = sx[None]
    tlist = np.array([0.0, 1.0, 2.0, 3.0])
    x = np.array([np.pi, 0.3, np.pi / 2 * 2])     # A = -i pi sigma_x (+ tiny drift) on steps 0 and 2
    psi0 = np.array([[1, 0]], complex)
    tgt = np.array([[0.6, 0.8j]], complex)
    Jr, Gr, taur = ref.evaluate(H0, Hc, tlist, x, psi0, tgt, gradient_method=ref.GRADGEN)
    monkeypatch.setenv("GRAPE_EXPM_T18", "0")     # the Pade kernels (the default exponential is the inverse-free polynomial)
    with g.GrapeHip(H0, Hc, tlist, psi0, tgt) as h:
        J, G, tau = h.eval(x)
        assert h.work()["pivoted_cells"] >= 2
    assert abs(J - Jr) <= TOL_J and abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr)
    monkeypatch.delenv("GRAPE_EXPM_T18")
    with g.GrapeHip(H0, Hc, tlist, psi0, tgt) as h:   # polynomial route: no denominator, nothing to pivot
        J, G, tau = h.eval(x)
        assert h.work()["pivoted_cells"] == 0 and h.work()["t18_cells"] == 3
    assert abs(J - Jr) <= TOL_J and abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr)
    # N = 64: a cyclic-shift generator (every diagonal tile of q(A) is badly conditioned)
    N = 64
    S = np.roll(np.eye(N), 1, axis=1)
    Hs = (S + S.T).astype(complex)
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 1, 3, 1, seed=5)
    pr["H0"] = (2.0 * Hs + 0.01 * pr["H0"][0])[None]
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"],
                                gradient_method=ref.TAYLOR)
    for t18 in ("0", "1"):
        monkeypatch.setenv("GRAPE_EXPM_T18", t18)
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"]) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            npiv = h.work()["pivoted_cells"]
        assert abs(J - Jr) <= TOL_J and abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr), (t18, npiv)
    monkeypatch.delenv("GRAPE_EXPM_T18")
    # blocked path (N > 64): a two-level pi-pulse embedded in a 70-level system zeroes two diagonal entries of q(A)
    N = 70
    pr = synth.make_problem(N, 1, 3, 2, seed=6)
    H0 = 0.3 * pr["H0"]
    H0[:, :2, :] = 0
    H0[:, :, :2] = 0
    H0[:, 0, 0], H0[:, 1, 1] = 1e-3, -1e-3
    Hc = np.zeros((1, N, N), complex)
    Hc[0, 0, 1] = Hc[0, 1, 0] = 1.0
    Hc[0, 2:, 2:] = 0.05 * pr["Hc"][0, 2:, 2:]
    x = np.array([np.pi, 0.3, np.pi])
    Jr, Gr, taur = ref.evaluate(H0, Hc, pr["tlist"], x, pr["psi0"], pr["target"], gradient_method=ref.TAYLOR)
    monkeypatch.setenv("GRAPE_EXPM_T18", "0")     # the order-13 Pade route of the blocked path (the default is the polynomial route)
    with g.GrapeHip(H0, Hc, pr["tlist"], pr["psi0"], pr["target"]) as h:
        J, G, tau = h.eval(x)
        npiv = h.work()["pivoted_cells"]
    monkeypatch.delenv("GRAPE_EXPM_T18")
    assert npiv >= 4
    assert abs(J - Jr) <= TOL_J and abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr), npiv
    # the polynomial route has no denominator: the same cells need no special treatment
    with g.GrapeHip(H0, Hc, pr["tlist"], pr["psi0"], pr["target"]) as h:
        J, G, tau = h.eval(x)
        w = h.work()
    assert w["pivoted_cells"] == 0 and w["t18_cells"] == 2 * 3
    assert abs(J - Jr) <= TOL_J and abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr)


def test_two_rank_sharded_device_path(g):
    """Two processes, each with its own trajectory shard and handle, real collectives (gloo on CUDA
    tensors: both ranks share the one GPU of this box) through ShardedEvaluator.eval_device -- the exact
    loop bench.py runs per rank with RCCL."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29541", os.path.join(root, "tools", "two_rank_gpu.py")]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "two-rank sharded device path OK" in res.stdout


@pytest.mark.parametrize("N,L,per_traj,functional", [(6, 2, False, 0), (16, 1, True, 2), (64, 2, False, 0), (100, 2, True, 1)])
def test_state_running_cost_expectation_family(g, ref, N, L, per_traj, functional):
    """g_b(Psi) = <Psi|D|Psi>, xi = -D Psi (test/test_state_running_cost.jl:32-40): J gains
    lambda_b * trapezoid(g_b) (optimize.jl:727-750, 764-766) and chi the inhomogeneity of :856-866,
    :897-908.  Checked against the C oracle and by finite differences of the GPU functional."""
    from grape_jl_amd import synth
    K, N_T, lam = 3, 7, 0.5
    pr = synth.make_problem(N, L, N_T, K, seed=500 + N, hermitian=(N != 6))
    pr["tlist"] = np.cumsum(np.concatenate([[0.0], 0.8 + 0.05 * np.arange(N_T)]))   # non-uniform grid
    rng = np.random.default_rng(N)
    def penalty():
        A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        return A @ A.conj().T / N
    D = np.stack([penalty() for _ in range(K)]) if per_traj else penalty()
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=functional,
                    D=D, lambda_b=lam) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        eps, fd = 1e-6, []
        for idx in (0, L * N_T - 1):
            xp, xm = pr["pulsevals"].copy(), pr["pulsevals"].copy()
            xp[idx] += eps
            xm[idx] -= eps
            fd.append((h.eval(xp, gradient=False)[0] - h.eval(xm, gradient=False)[0]) / (2 * eps) - G[idx])
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                functional=functional, gradient_method=ref.TAYLOR, D=D, lambda_b=lam)
    assert abs(J - Jr) <= 1e-12 * max(1.0, abs(Jr))
    assert np.abs(tau - taur).max() <= TOL_TAU
    assert np.abs(G - Gr).max() <= tol_G(Gr)
    assert np.abs(fd).max() <= 1e-7 * max(1.0, np.abs(Gr).max())


@pytest.mark.parametrize("N,K", [(256, 3), (256, 9), (256, 17), (256, 33), (128, 2), (128, 20), (100, 40)])
def test_cooperative_sweeps_all_slice_shapes(g, ref, N, K, monkeypatch):
    """Few large trajectories: S workgroups share one trajectory in the sweeps (sweep_coop_kernel); K selects
    the slice height R = NP/S in {4, 8, 16, 32, 64}.  Same parity bar as everywhere (optimize.jl:731-738, 881),
    and agreement with the one-workgroup-per-trajectory kernel."""
    from grape_jl_amd import synth
    L, N_T = 2, 5
    pr = synth.make_problem(N, L, N_T, K, seed=900 + N + K, hermitian=(K % 2 == 1))
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args, functional=1) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        fw = h.storage(0)
    monkeypatch.setenv("GRAPE_SWEEP_COOP", "0")
    with g.GrapeHip(*args, functional=1) as h:
        J1, G1, tau1 = h.eval(pr["pulsevals"])
        fw1 = h.storage(0)
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                functional=1, gradient_method=ref.TAYLOR)
    assert np.abs(fw - fw1).max() <= 1e-14
    assert abs(J - J1) <= 1e-14 and np.abs(G - G1).max() <= 1e-13 * max(1.0, np.abs(G1).max())
    assert abs(J - Jr) <= 1e-12 and np.abs(tau - taur).max() <= TOL_TAU
    assert np.abs(G - Gr).max() <= tol_G(Gr)


@pytest.mark.parametrize("N", [6, 64, 100])
def test_trajectories_with_identical_generators_share_propagators(g, ref, N, monkeypatch):
    """Gate-optimisation layout: several initial states under the SAME Hamiltonian (reference: one Trajectory
    per basis state with the same generator, docs/src/tutorial.md:365-372).  The exponentials depend on
    (generator, time step) only, so they are computed once per distinct generator; results are unchanged."""
    from grape_jl_amd import synth
    K, L, N_T = 6, 2, 5
    pr = synth.make_problem(N, L, N_T, K, seed=77 + N)
    pr["H0"][2] = pr["H0"][0]
    pr["H0"][3] = pr["H0"][0]
    pr["H0"][5] = pr["H0"][1]          # classes: {0,2,3}, {1,5}, {4}
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    # (bit-for-bit only with the same arithmetic on both sides: one propagator per trajectory lets the walks of the assembly
    # kernel carry the states along -- round 5 -- which shared propagators cannot; that comparison follows, to rounding)
    monkeypatch.setenv("GRAPE_EXPM_WALK", "0")
    with g.GrapeHip(*args) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        w = h.work()
        U3, U0 = h.propagator(3, 2), h.propagator(0, 2)
    assert w["expm_cells"] == 3 * N_T and w["cells"] == K * N_T
    assert np.array_equal(U3, U0)
    monkeypatch.setenv("GRAPE_NO_DEDUP", "1")
    with g.GrapeHip(*args) as h:
        J1, G1, tau1 = h.eval(pr["pulsevals"])
        assert h.work()["expm_cells"] == K * N_T
    assert J == J1 and np.array_equal(G, G1) and np.array_equal(tau, tau1)
    monkeypatch.delenv("GRAPE_EXPM_WALK")
    with g.GrapeHip(*args) as h:
        J2, G2, tau2 = h.eval(pr["pulsevals"])
    assert abs(J - J2) <= 1e-14 and np.abs(tau - tau2).max() <= 1e-14 and np.abs(G - G2).max() <= 1e-13 * max(np.abs(G).max(), 1e-3)
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                gradient_method=ref.TAYLOR)
    assert abs(J - Jr) <= TOL_J and np.abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr)


@pytest.mark.parametrize("N", [40, 64, 130])
def test_hermitian_fast_path_matches_general_path(g, N, monkeypatch):
    """Hermitian generators let phase A skip the mirrored tiles / blocks of the powers and use the Chebyshev coefficient
    set with the spectral scaling, where general matrices (GRAPE_NO_HERM=1) take the Taylor set with the norm-based
    scaling: the two must give the same propagators and gradient to rounding -- two different approximants, each at
    the 2e-14 * max(1, dt) of test_expm_kernel_vs_scipy."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, 6, 3, seed=4242 + N, dt=1.7)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        U = h.propagator(1, 3)
    monkeypatch.setenv("GRAPE_NO_HERM", "1")
    with g.GrapeHip(*args) as h:
        J1, G1, tau1 = h.eval(pr["pulsevals"])
        U1 = h.propagator(1, 3)
    assert np.abs(U - U1).max() <= 2e-14 * 1.7
    assert np.abs(U.conj().T @ U - np.eye(N)).max() <= 1e-13
    assert abs(J - J1) <= 1e-14 and np.abs(tau - tau1).max() <= 1e-13
    assert np.abs(G - G1).max() <= 1e-13 * max(1.0, np.abs(G1).max())


def test_order13_certificate_matches_measured_norm_path(g, monkeypatch):
    """expm_single skips the 1-norm of a cell when dt (||H0_k||_1 + sum_l |eps_l| ||H_l||_1) already certifies order 13
    without squaring; GRAPE_NORM_BOUND=0 always measures the norm.  Cells whose true norm is below 2.1 while the bound
    is above it get order 13 instead of 9 -- the propagators agree to rounding."""
    from grape_jl_amd import synth
    pr = synth.make_problem(64, 2, 12, 3, seed=21, dt=0.55)        # ||A||_1 around the 2.1 threshold
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        U = h.propagator(1, 5)
    monkeypatch.setenv("GRAPE_NORM_BOUND", "0")
    with g.GrapeHip(*args) as h:
        J0, G0, tau0 = h.eval(pr["pulsevals"])
        U0 = h.propagator(1, 5)
    assert np.abs(U - U0).max() <= 5e-15
    assert abs(J - J0) <= 1e-14 and np.abs(tau - tau0).max() <= 1e-14
    assert np.abs(G - G0).max() <= 1e-13 * max(np.abs(G0).max(), 1e-3)


@pytest.mark.parametrize("prop", [0, 1], ids=["expprop", "series"])
@pytest.mark.parametrize("cid", ["C1", "C2"])
def test_baseline_configs_c1_c2_full_parity(g, ref, cid, prop):
    """BASELINE.json configs 1 and 2 at full size against the C oracle's literal :gradgen route: the README two-level
    problem (500 steps, closed form J_T = 1 - (0.04/1.04) sin^2(5 sqrt(1.04))) and N = 16, 1 control, 500 steps,
    32 trajectories -- every stored quantity, both propagators."""
    from grape_jl_amd import synth
    pr = synth.make_config(cid)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args, prop_method=prop) as h:
        J, G, tau, psiT = h.eval(pr["pulsevals"], want_psiT=True)
        tg = h.tau_grads()
    Jr, Gr, taur, parts = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], gradient_method=ref.GRADGEN, want_parts=True)
    assert abs(J - Jr) <= TOL_J and np.abs(tau - taur).max() <= TOL_TAU and np.abs(G - Gr).max() <= tol_G(Gr)
    assert np.abs(psiT - parts["psiT"]).max() <= 1e-12
    assert np.abs(tg - parts["tau_grads"]).max() <= 1e-10 * max(np.abs(parts["tau_grads"]).max(), 1e-3)
    if cid == "C1":
        assert abs(J - (1.0 - (0.04 / 1.04) * np.sin(5.0 * np.sqrt(1.04)) ** 2)) <= 1e-12
        assert abs(G[0] - 1.3367344501042e-3) <= 1e-13 and abs(G[249] - 3.5455160183374e-3) <= 1e-13   # SURVEY 8c probe


def test_baseline_config_c5_shard_properties(g):
    """BASELINE.json config 5 (N = 256, 4 controls, 2000 steps) on a 2-trajectory slice of a GPU's shard (the oracle
    is far too slow at this size): J from tau, norm conservation of all stored states, gradient vs central finite
    differences of the GPU functional, and repeatability."""
    from grape_jl_amd import synth
    pr = synth.make_config("C5", K=2)
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"]) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        assert abs(J - (1 - abs(tau.sum()) ** 2 / 4)) <= 1e-14
        assert np.abs(np.linalg.norm(h.storage(0), axis=2) - 1.0).max() <= 1e-11
        assert np.abs(np.linalg.norm(h.storage(1), axis=2) - 1.0).max() <= 1e-11
        eps = 1e-5
        for idx in (3, 2000 + 1234, 4 * 2000 - 1):
            xp, xm = pr["pulsevals"].copy(), pr["pulsevals"].copy()
            xp[idx] += eps
            xm[idx] -= eps
            fd = (h.eval(xp, gradient=False)[0] - h.eval(xm, gradient=False)[0]) / (2 * eps)
            assert abs(fd - G[idx]) <= 5e-10 + 1e-5 * abs(G[idx])
        J2, G2, _ = h.eval(pr["pulsevals"])
        assert J2 == J and np.array_equal(G2, G)


def test_bench_contract_two_rank_rehearsal(g):
    """PLAIN `python bench.py --gpus 2` -- no launcher in the test (round-5 review: `--gpus` used to be parsed and ignored, so
    this form ran one rank and printed n_gpus = 1): bench.py starts the two ranks itself, as a child
    `python -m torch.distributed.run`, before it touches torch or the GPU.  Rehearsal mode: both ranks on this box's one
    GPU, gloo collectives (the driver's N > 1 runs use RCCL on one GPU per rank).  stdout carries exactly ONE line, a JSON
    object with the contract's keys; the whole-job value counts both shards; the all-reduce latency is reported."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["GRAPE_BENCH_REHEARSAL"] = "1"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full",
           "--no-cpu-baseline"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout[:2000]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["scaling"] == "weak" and d["dtype"] == "f64"
    assert abs(d["value"] - 2 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]
    assert d["roofline"]["bound"] == "mfma" and 0.0 < d["roofline"]["frac"] < 1.0
    assert d["gradient_allreduce_latency_us"] > 0.0
    assert d["phase_b"]["GB_per_s"] is None or d["phase_b"]["GB_per_s"] <= 8000.0      # never above the HBM peak
    # a launcher whose WORLD_SIZE disagrees with --gpus: refused before anything is measured
    env_bad = dict(env, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=root, env=env_bad)
    assert bad.returncode != 0 and not bad.stdout.strip() and "WORLD_SIZE" in bad.stderr


def test_bench_contract_four_rank_rehearsal_of_config_c4(g):
    """BASELINE config 4 (128 trajectories per GPU, one rank per GPU) rehearsed with as many ranks as this pool lets one
    box run against its one GPU: SIX processes may have the card open at once, and this test process and the launcher
    are two of them (a six-rank attempt was killed by the box's process guard: eight processes on the GPU) -- so the
    driver's 8-rank launch is rehearsed with FOUR (`bench.py --gpus 4 --config C4` under torch.distributed.run, 512
    trajectories, gloo collectives, every rank on device 0).  One JSON line with n_gpus = 4, and the functional value the
    ranks agree on -- formed from the all-reduced sums of four shard handles in four processes -- equals the value ONE
    handle with all 512 trajectories returns, to 1e-14."""
    import json
    import subprocess
    import sys
    from grape_jl_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GRAPE_BENCH_REHEARSAL="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr",
           "127.0.0.1", "--master-port", "29547", os.path.join(root, "bench.py"), "--gpus", "4", "--config", "C4",
           "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout[:2000]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4 and d["scaling"] == "weak" and "512 total" in d["config"]["workload"]
    assert abs(d["value"] - 4 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]
    assert d["gradient_allreduce_latency_us"] > 0.0
    # the same 512 trajectories (rank r owns [128 r, 128 (r + 1)), synth.make_config(k_offset = 128 r)) behind ONE handle
    prs = [synth.make_config("C4", K=128, k_offset=128 * r) for r in range(4)]
    cat = lambda key: np.concatenate([p[key] for p in prs])      # noqa: E731
    with g.GrapeHip(cat("H0"), prs[0]["Hc"], prs[0]["tlist"], cat("psi0"), cat("target"), cat("weights")) as h:
        J1, _, _ = h.eval(prs[0]["pulsevals"])
    assert abs(d["J"] - J1) <= 1e-14, (d["J"], J1)


def test_bench_plain_run_and_dump_outputs(g, tmp_path):
    """A plain `bench.py --dump-outputs DIR` (config C2, one GPU): one JSON line with the headline keys and without what
    --full adds; DIR holds J, G, tau_re and tau_im as float64 -- what grape_eval returned for the pulses of the last timed
    step (bench.py's seeded perturbation, regenerated here) -- and a second run with the same arguments writes the same."""
    import json
    import subprocess
    import sys
    from grape_jl_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    steps, warmup = 3, 2
    dumps = []
    for run in ("a", "b"):
        out_dir = tmp_path / run
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--config", "C2", "--steps", str(steps),
               "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root, env=env)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, res.stdout[:2000]
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "roofline"):
            assert key in d
        assert d["steps"] == steps and d["warmup"] == warmup and d["dtype"] == "f64" and d["higher_is_better"] is True
        assert abs(d["value"] - steps / (d["ms_per_step"] * steps * 1e-3)) <= 1e-6 * d["value"]
        for key in ("device_resident_loop", "J", "matrix_free", "cpu_baseline", "speedup_vs_cpu_baseline"):
            assert key not in d
        arrs = {name: np.load(out_dir / f"{name}.npy") for name in ("J", "G", "tau_re", "tau_im")}
        assert all(a.dtype == np.float64 for a in arrs.values())
        dumps.append(arrs)
    pr = synth.make_config("C2")
    N, L, N_T, K = synth.CONFIGS["C2"]
    rng = np.random.default_rng(12345)
    xs = [pr["pulsevals"] + 1e-3 * (rng.random(L * N_T) - 0.5) for _ in range(warmup + steps)]
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], functional=g.J_T_SM,
                    gradient_method=g.GRAD_GRADGEN, K_total=K) as h:
        J, G, tau = h.eval(xs[-1])
    for arrs in dumps:
        assert arrs["J"].shape == (1,) and arrs["G"].shape == (L * N_T,) and arrs["tau_re"].shape == (K,)
        assert abs(arrs["J"][0] - J) <= 1e-14
        assert np.abs(arrs["G"] - G).max() <= 1e-12 * max(np.abs(G).max(), 1e-3)
        assert np.abs(arrs["tau_re"] + 1j * arrs["tau_im"] - tau).max() <= 1e-14
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name


@pytest.mark.parametrize("N,herm", [(33, True), (40, False), (48, True)])
def test_three_tile_instantiation_matches_padded_four_tile_path(g, ref, N, herm, monkeypatch):
    """33 <= N <= 48 runs on three 16-wide tiles (NP = 48: expm_pade_kernel<3>, three-wave sweeps, deriv2_kernel<48>)
    instead of being padded to 64 (GRAPE_NO_NT3=1 restores the padding): same results to rounding, and the oracle's."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, 9, 3, seed=300 + N, hermitian=herm, dt=1.3)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args) as h3:
        J3, G3, tau3 = h3.eval(pr["pulsevals"])
        U3 = h3.propagator(1, 4)
        fw3, bw3 = h3.storage(0), h3.storage(1)
    monkeypatch.setenv("GRAPE_NO_NT3", "1")
    with g.GrapeHip(*args) as h4:
        J4, G4, tau4 = h4.eval(pr["pulsevals"])
        U4 = h4.propagator(1, 4)
        fw4 = h4.storage(0)
    monkeypatch.delenv("GRAPE_NO_NT3")
    assert np.abs(U3 - U4).max() <= 5e-15
    assert abs(J3 - J4) <= 1e-14 and np.abs(tau3 - tau4).max() <= 1e-14 and np.abs(fw3 - fw4).max() <= 1e-13
    assert np.abs(G3 - G4).max() <= 1e-13 * max(np.abs(G4).max(), 1e-3)
    Jr, Gr, taur = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:])
    assert abs(J3 - Jr) <= TOL_J and np.abs(tau3 - taur).max() <= TOL_TAU and np.abs(G3 - Gr).max() <= tol_G(Gr)
    assert np.abs(np.linalg.norm(bw3, axis=2) - 1.0).max() <= 1e-12 or not herm


@pytest.mark.parametrize("N,L,K,N_T,dt,herm", [
    (6, 2, 2, 5, 20.0, True), (20, 1, 2, 4, 25.0, False), (40, 2, 2, 3, 20.0, True), (64, 2, 3, 20, 18.0, True),
    (64, 3, 2, 3, 60.0, True), (100, 2, 2, 3, 20.0, True)])
def test_exact_gradient_route_is_accurate_for_large_norm_steps(g, ref, N, L, K, N_T, dt, herm):
    """gradient_method = :gradgen at ||H|| dt ~ 20-70 per time step.  The reference's gradient-generator route goes
    through the scaled-and-squared dense block exponential and is accurate for any norm; the HIP path sums the series
    of that exponential on the extended vector and therefore cuts such a step into sub-steps (deriv_substeps: the
    gradient slots are carried from one sub-step to the next).  Without them the unscaled series loses
    eps * exp(||H|| dt) -- 1e-8 at 20, nothing at 40 -- or runs out of orders (GRAPE_ERR_TAYLOR).  Mixed problem: only
    SOME time steps are long (non-uniform grid), so batches with and without sub-steps sit side by side."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=900 + N, dt=1.0, hermitian=herm)
    tl = np.concatenate([[0.0], np.cumsum(np.where(np.arange(N_T) % 3 == 1, dt, 0.7))])   # every third step is long
    args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"])
    with g.GrapeHip(*args) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        tg = h.tau_grads()
        orders = h.work()["deriv_orders"]
    Jr, Gr, taur, parts = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], want_parts=True)
    assert abs(J - Jr) <= 1e-11 and np.abs(tau - taur).max() <= 1e-11     # 1e-16 * ||A||_1 * squarings on both sides
    assert np.abs(G - Gr).max() <= tol_G(Gr) * 10                          # (the oracle's own error grows with the norm)
    assert np.abs(tg - parts["tau_grads"]).max() <= 1e-9 * max(np.abs(parts["tau_grads"]).max(), 1e-3)
    assert orders > 0


def test_taylor_route_keeps_the_reference_behaviour_for_large_norm_steps(g):
    """gradient_method = :taylor is the reference's plain recursion (optimize.jl:604-653): no sub-steps; a step whose
    series does not converge within taylor_grad_max_order raises the reference's error."""
    from grape_jl_amd import synth
    pr = synth.make_problem(16, 1, 3, 1, seed=3, dt=60.0)
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], gradient_method=g.GRAD_TAYLOR) as h:
        with pytest.raises(g.GrapeHipError) as ei:
            h.eval(pr["pulsevals"])
        assert ei.value.code == -5
    with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"]) as h:   # :gradgen works
        J, G, _ = h.eval(pr["pulsevals"])
        assert np.isfinite(G).all()


def test_persistent_phase_a_matches_per_cell_launch_and_keeps_the_pivoted_fallback(g, ref, monkeypatch):
    """N = 64 with enough cells for the persistent expm kernel (one workgroup per CU walking its cells, the next cell's A
    formed under the first tile inversion): identical to the one-workgroup-per-cell launch (GRAPE_EXPM_PERSIST=0) bit
    for bit, including cells that are flagged for the pivoted Pade solve, mixed Pade orders (non-uniform grid: some
    steps are short enough for orders 7/9, one is long enough for a squaring) and a non-Hermitian generator set."""
    from grape_jl_amd import synth
    for herm in (True, False):
        N, L, N_T, K = 64, 2, 560, 2                     # 1120 cells >= 4 x 256
        pr = synth.make_problem(N, L, N_T, K, seed=50 + herm, hermitian=herm)
        dts = np.ones(N_T)
        dts[5::50] = 0.2                                  # lower Pade orders (norm certificate does not apply)
        dts[7::100] = 3.0                                 # one squaring
        tl = np.concatenate([[0.0], np.cumsum(dts)])
        if herm:
            # a two-level pi-pulse embedded in the 64-level system zeroes two diagonal entries of q(A) in the steps where
            # control 0 has the value pi: those cells must go through the pivoted solve
            pr["H0"][:, :2, :] = 0
            pr["H0"][:, :, :2] = 0
            pr["H0"][:, 0, 0], pr["H0"][:, 1, 1] = 1e-3, -1e-3
            Hc0 = np.zeros((N, N), complex)
            Hc0[0, 1] = Hc0[1, 0] = 1.0
            Hc0[2:, 2:] = 0.05 * pr["Hc"][0, 2:, 2:]
            pr["Hc"][0] = Hc0
            pr["Hc"][1, :2, :] = 0
            pr["Hc"][1, :, :2] = 0
            pr["pulsevals"][[3, 300, 559]] = np.pi
        args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"])
        # Hermitian generators take the inverse-free polynomial kernel by default: the Pade kernels are selected with
        # GRAPE_EXPM_T18=0 (read at grape_create), and the default path is compared with them below
        monkeypatch.setenv("GRAPE_EXPM_T18", "0")
        with g.GrapeHip(*args) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            w = h.work()
            U = h.propagator(1, 7)
        monkeypatch.setenv("GRAPE_EXPM_PERSIST", "0")
        with g.GrapeHip(*args) as h0:
            J0, G0, tau0 = h0.eval(pr["pulsevals"])
            w0 = h0.work()
            U0 = h0.propagator(1, 7)
        monkeypatch.delenv("GRAPE_EXPM_PERSIST")
        monkeypatch.delenv("GRAPE_EXPM_T18")
        assert J == J0 and np.array_equal(G, G0) and np.array_equal(tau, tau0) and np.array_equal(U, U0)
        if herm:
            # the polynomial kernel on the same problem -- pi-pulse cells (no denominator: nothing to pivot), short steps,
            # the step that needs a squaring in the Pade route: same credited work, results equal to rounding
            with g.GrapeHip(*args) as ht:
                Jt, Gt, taut = ht.eval(pr["pulsevals"])
                wt = ht.work()
                Ut = np.stack([ht.propagator(1, n) for n in (3, 5, 7, 300)])
            assert wt["t18_cells"] == K * N_T and wt["pivoted_cells"] == 0
            assert wt["flop_expm"] == w["flop_expm"] and wt["squarings"] == w["squarings"]
            assert abs(Jt - J) <= TOL_J and np.abs(taut - tau).max() <= TOL_TAU and np.abs(Gt - G).max() <= tol_G(G)
            monkeypatch.setenv("GRAPE_EXPM_T18", "0")
            with g.GrapeHip(*args) as hp:
                hp.eval(pr["pulsevals"])
                Up = np.stack([hp.propagator(1, n) for n in (3, 5, 7, 300)])
            monkeypatch.delenv("GRAPE_EXPM_T18")
            assert np.abs(Ut - Up).max() <= 2e-14
            assert np.abs(np.einsum("nij,nik->njk", Ut.conj(), Ut) - np.eye(N)).max() <= 1e-13
        assert w["squarings"] == w0["squarings"] > 0 and w["pivoted_cells"] == w0["pivoted_cells"]
        assert w["flop_expm"] == w0["flop_expm"]
        if herm:
            assert w["pivoted_cells"] >= 2 * 3             # the three pi-pulse steps of both trajectories
        # a sample of the first steps against the oracle (the full problem is too slow for the dense block exponential)
        ns = 12
        xs = pr["pulsevals"].reshape(L, N_T)[:, :ns].reshape(-1)
        with g.GrapeHip(pr["H0"], pr["Hc"], tl[: ns + 1], pr["psi0"], pr["target"], pr["weights"]) as hs:
            Js, Gs, taus = hs.eval(xs)
        Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], tl[: ns + 1], xs, pr["psi0"], pr["target"], pr["weights"],
                                    gradient_method=ref.TAYLOR)
        assert abs(Js - Jr) <= TOL_J and np.abs(taus - taur).max() <= TOL_TAU and np.abs(Gs - Gr).max() <= tol_G(Gr)
        assert np.abs(np.linalg.norm(U, axis=0) - 1.0).max() <= 1e-12 or not herm


@pytest.mark.parametrize("case", range(6))
def test_exponential_paths_differential_on_random_grids(g, ref, case, monkeypatch):
    """The N = 64 exponential in all its forms on random problems with non-uniform time grids whose step sizes reach every
    Pade order and up to three squarings: persistent kernel == one-workgroup-per-cell kernel bit for bit (both run the
    look-ahead solve on rotated strips, split squares, late-arriving mirrored tiles), Hermitian fast path == general path
    (GRAPE_NO_HERM=1) to rounding, and the evaluation against the C restatement (tools/diff_paths.py is the long form)."""
    from grape_jl_amd import synth
    rng = np.random.default_rng(977 + case)
    N = (64, 64, 60, 49, 64, 64)[case]
    K = 9 if case % 2 else 5          # 9 x 120 cells: persistent kernel; 5 x 120: per-cell kernel by size
    N_T, L = 120, 2
    pr = synth.make_problem(N, L, N_T, K, seed=int(rng.integers(1 << 30)))
    scale = (0.02, 0.2, 1.0, 6.0, 2.5, 0.6)[case]
    tl = np.concatenate([[0.0], np.cumsum(scale * (0.5 + rng.random(N_T)))])
    args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"])
    res = {}
    for name, env in (("t18", {}), ("persist", {"GRAPE_EXPM_T18": "0"}),
                      ("percell", {"GRAPE_EXPM_T18": "0", "GRAPE_EXPM_PERSIST": "0"}), ("general", {"GRAPE_NO_HERM": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with g.GrapeHip(*args) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            res[name] = (J, G.copy(), np.stack([h.propagator(0, n) for n in (0, N_T // 2, N_T - 1)]))
        for k in env:
            monkeypatch.delenv(k)
    assert res["persist"][0] == res["percell"][0] and np.array_equal(res["persist"][1], res["percell"][1])
    assert np.array_equal(res["persist"][2], res["percell"][2])
    # the inverse-free polynomial kernel (default for Hermitian generators, N > 32) against the Pade kernel
    assert abs(res["t18"][0] - res["persist"][0]) <= TOL_J
    assert np.abs(res["t18"][1] - res["persist"][1]).max() <= tol_G(res["persist"][1])
    assert np.abs(res["t18"][2] - res["persist"][2]).max() <= 1e-12
    assert abs(res["persist"][0] - res["general"][0]) <= TOL_J
    assert np.abs(res["persist"][1] - res["general"][1]).max() <= tol_G(res["general"][1])
    assert np.abs(res["persist"][2] - res["general"][2]).max() <= 1e-12
    Jr, Gr, taur = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:], gradient_method=ref.TAYLOR)
    assert abs(res["persist"][0] - Jr) <= TOL_J and np.abs(res["persist"][1] - Gr).max() <= tol_G(Gr)
    assert abs(res["t18"][0] - Jr) <= TOL_J and np.abs(res["t18"][1] - Gr).max() <= tol_G(Gr)


@pytest.mark.parametrize("N", (64, 48, 32))
def test_four_product_route_hands_cells_beyond_its_bound_to_the_five_product_route(g, ref, N, monkeypatch):
    """Hermitian generators, 16 < N <= 64: the degree-16 four-product polynomial (grape_t18.hip.h, expm_t16_cell) is valid for
    spectral radii up to 1.36 and proves that per cell from sum lam^8; cells beyond the bound are listed and redone by the
    degree-18 five-product launch behind it.  A time grid with mostly unit steps and some steps of 2.0 and 2.5 mixes both
    kinds: every cell is exponentiated exactly once as far as the counters go, results agree with the five-product route
    alone (GRAPE_EXPM_T16=0), with the Pade route and with the C restatement."""
    from grape_jl_amd import synth
    # (round 5: the assembly kernel of N > 48 would keep the long cells -- scaling and squaring around its four products,
    # tests/test_gpu_asm.py::test_scaled_four_product_route_* -- this test is about the hand-over, which stays the way of the
    # compiled kernels and of cells whose planned scaling turns out too small)
    monkeypatch.setenv("GRAPE_EXPM_SQ", "0")
    L, N_T, K = 2, 300, 4                               # 1200 cells >= 4 x 256: persistent grid with several cells per workgroup
    pr = synth.make_problem(N, L, N_T, K, seed=1600 + N)
    dts = np.ones(N_T)
    dts[3::7] = 2.0
    dts[5::11] = 2.5
    tl = np.concatenate([[0.0], np.cumsum(dts)])
    args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"])
    sample = [(0, 0), (1, 3), (2, 5), (3, N_T - 1), (1, 10), (2, 16)]
    res = {}
    for name, env in (("t16", {}), ("t18", {"GRAPE_EXPM_T16": "0"}), ("pade", {"GRAPE_EXPM_T18": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with g.GrapeHip(*args) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            res[name] = (J, G.copy(), tau.copy(), np.stack([h.propagator(k, n) for k, n in sample]), h.work())
            Jrep, Grep, _ = h.eval(pr["pulsevals"])          # the same pulses: the same route, the same bits
            assert Jrep == J and np.array_equal(Grep, G) and h.work()["t16_cells"] == res[name][4]["t16_cells"]
        for k in env:
            monkeypatch.delenv(k)
    w = res["t16"][4]
    big = int((dts > 1.5).sum()) * K
    assert w["t18_cells"] == K * N_T                       # every cell counted once: four-product cells + redone cells
    assert 0 < w["t16_cells"] <= K * N_T - big             # no cell with a step of 2.0 or more passes the bound (rho dt >= 1.4)
    assert w["t16_cells"] >= 0.8 * (K * N_T - big)         # ... and the unit steps do (rho about 1, bound about 1.2)
    assert res["t18"][4]["t16_cells"] == 0
    assert w["flop_expm"] == res["t18"][4]["flop_expm"] == res["pade"][4]["flop_expm"]     # credited work: route-independent
    for other in ("t18", "pade"):
        assert abs(res["t16"][0] - res[other][0]) <= TOL_J
        assert np.abs(res["t16"][1] - res[other][1]).max() <= tol_G(res[other][1])
        assert np.abs(res["t16"][2] - res[other][2]).max() <= TOL_TAU
        assert np.abs(res["t16"][3] - res[other][3]).max() <= 1e-14
    U = res["t16"][3]
    assert np.abs(np.einsum("nij,nik->njk", U.conj(), U) - np.eye(N)).max() <= 5e-15
    ns = 12
    xs = pr["pulsevals"].reshape(L, N_T)[:, :ns].reshape(-1)
    with g.GrapeHip(pr["H0"], pr["Hc"], tl[: ns + 1], pr["psi0"], pr["target"], pr["weights"]) as hs:
        Js, Gs, taus = hs.eval(xs)
        assert 0 < hs.work()["t16_cells"] < K * ns
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], tl[: ns + 1], xs, pr["psi0"], pr["target"], pr["weights"],
                                gradient_method=ref.TAYLOR)
    assert abs(Js - Jr) <= TOL_J and np.abs(taus - taur).max() <= TOL_TAU and np.abs(Gs - Gr).max() <= tol_G(Gr)


def test_four_product_route_is_planned_from_the_pulses_alone(g, monkeypatch):
    """Whether the four-product route is tried is decided per evaluation on the device, from the pulse values (t16_plan_kernel:
    a spectral-radius estimate from the Gram matrices of the operators) -- never from what the handle evaluated before
    (round-3 advisor finding).  With more than a quarter of the cells predicted beyond the bound the route is skipped: no
    cell is exponentiated twice and the work is that of the five-product route alone (GRAPE_EXPM_T16=0: same kernel, same
    cell function).  The same pulses give the same bits whatever was evaluated in between."""
    from grape_jl_amd import synth
    # (round 5: with scaling and squaring around the four products the assembly kernel keeps cells up to a radius of ~ 9 and
    # the route is skipped only beyond that; the decision logic under test is the same -- here without the scaling)
    monkeypatch.setenv("GRAPE_EXPM_SQ", "0")
    N, L, N_T, K = 64, 2, 300, 4
    pr = synth.make_problem(N, L, N_T, K, seed=1664)
    tl = np.arange(N_T + 1) * 1.8                        # every cell beyond 1.36
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"]) as h:
        J1, G1, tau1 = h.eval(pr["pulsevals"])
        w1 = h.work()
        J2, G2, tau2 = h.eval(pr["pulsevals"])
        w2 = h.work()
    monkeypatch.setenv("GRAPE_EXPM_T16", "0")
    with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"]) as h:
        J0, G0, tau0 = h.eval(pr["pulsevals"])
        w0 = h.work()
    monkeypatch.delenv("GRAPE_EXPM_T16")
    assert w1["t16_cells"] == 0 and w1["t18_cells"] == K * N_T and w2["t16_cells"] == 0 and w2["t18_cells"] == K * N_T
    assert w1["t18_mfma_flop"] == w2["t18_mfma_flop"] == w0["t18_mfma_flop"]      # skipped from the FIRST evaluation on
    assert w1["flop_expm"] == w0["flop_expm"]
    assert J1 == J2 and np.array_equal(G1, G2) and np.array_equal(tau1, tau2)
    # (against the handle without the route: equal up to the rounding of H0 + S_n, the summed controls this handle's
    # kernels fetch, against H0 + eps_1 H_1 + eps_2 H_2)
    assert abs(J1 - J0) <= 1e-13 and np.abs(G1 - G0).max() <= 1e-13 * max(np.abs(G0).max(), 1e-3) and np.abs(tau1 - tau0).max() <= 1e-13
    # pulses inside the range, pulses beyond it (the controls scaled up: the route is skipped), the first pulses again
    tl1 = np.arange(N_T + 1) * 1.0
    big = 8.0 * pr["pulsevals"]
    with g.GrapeHip(pr["H0"], pr["Hc"], tl1, pr["psi0"], pr["target"], pr["weights"]) as h:
        Ja, Ga, _ = h.eval(pr["pulsevals"])
        wa = h.work()
        Jb, Gb, _ = h.eval(big)
        wb = h.work()
        Jc, Gc, _ = h.eval(pr["pulsevals"])
        wc = h.work()
    with g.GrapeHip(pr["H0"], pr["Hc"], tl1, pr["psi0"], pr["target"], pr["weights"]) as h:
        Jd, Gd, _ = h.eval(big)
    assert wa["t16_cells"] == K * N_T and wb["t16_cells"] == 0 and wc["t16_cells"] == K * N_T
    assert Ja == Jc and np.array_equal(Ga, Gc) and wa["t18_mfma_flop"] == wc["t18_mfma_flop"]
    assert Jb == Jd and np.array_equal(Gb, Gd)


@pytest.mark.parametrize("N,L,N_T,K", [(64, 2, 300, 4), (48, 1, 203, 3), (60, 2, 129, 9), (40, 2, 64, 130), (48, 4, 100, 3),
                                      (36, 5, 50, 2), (64, 3, 100, 3), (64, 4, 70, 2), (60, 5, 50, 2), (64, 6, 129, 2)])
def test_derivative_kernel_with_one_wave_per_batch_matches_the_shared_batch_kernel(g, ref, N, L, N_T, K, monkeypatch):
    """Hermitian operators, 32 < N <= 64, L <= 2 (N <= 48: L <= 5): deriv3_kernel (grape_deriv3.hip.h: one wave per batch of 16 cells, operators
    as upper-triangle tiles in LDS, mirrored tiles through the negation bit of the matrix instruction; at four tiles per
    side the assembly kernels of asm/gen_d3.py and, for three to eight controls, asm/gen_d3s.py) against deriv2_kernel
    (GRAPE_DERIV3=0) on the same inputs -- same series, same stopping rule, the additions of a cell in the same order: equal
    to rounding; and both against the C restatement on the first steps.  Shapes: a last batch with unused columns, padded
    sizes (60 -> 64, 40 -> 48), more trajectories than workgroups, several workgroups per trajectory, shaped amplitudes."""
    from grape_jl_amd import synth
    monkeypatch.setenv("GRAPE_DERIV_ECON", "0")     # (twins of the Taylor sum; the economized series: tests/test_gpu_asm.py)
    pr = synth.make_problem(N, L, N_T, K, seed=3300 + N + L)
    rng = np.random.default_rng(N * 7 + L)
    tl = np.concatenate([[0.0], np.cumsum(0.6 + 0.8 * rng.random(N_T))])
    shape = 0.5 + rng.random((L, N_T))
    res = {}
    for name, env in (("d3", {}), ("d2", {"GRAPE_DERIV3": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with g.GrapeHip(pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"], shape=shape) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            res[name] = (J, G.copy(), tau.copy(), h.work())
        for k in env:
            monkeypatch.delenv(k)
    assert res["d3"][0] == res["d2"][0] and np.array_equal(res["d3"][2], res["d2"][2])       # the sweeps are the same code
    assert np.abs(res["d3"][1] - res["d2"][1]).max() <= 1e-13 * max(np.abs(res["d2"][1]).max(), 1e-3)
    if N > 48 and L > 2:     # streamed controls: the four batches of a workgroup stop together (never earlier than each alone)
        assert res["d2"][3]["deriv_orders"] <= res["d3"][3]["deriv_orders"] <= res["d2"][3]["deriv_orders"] + K * N_T
    else:
        assert res["d3"][3]["deriv_orders"] == res["d2"][3]["deriv_orders"] > 0                # same stopping decisions
    ns = 10
    xs = pr["pulsevals"].reshape(L, N_T)[:, :ns].reshape(-1)
    Ks = min(K, 3)
    with g.GrapeHip(pr["H0"][:Ks], pr["Hc"], tl[: ns + 1], pr["psi0"][:Ks], pr["target"][:Ks], pr["weights"][:Ks],
                    shape=shape[:, :ns]) as hs:
        Js, Gs, taus = hs.eval(xs)
    import grape_oracle as go    # (the numpy restatement knows shaped amplitudes)
    Jr, Gr, taur = go.evaluate_gradient(pr["H0"][:Ks], pr["Hc"], tl[: ns + 1], xs, pr["psi0"][:Ks], pr["target"][:Ks],
                                        pr["weights"][:Ks], shape=shape[:, :ns])
    assert abs(Js - Jr) <= TOL_J and np.abs(taus - taur).max() <= TOL_TAU and np.abs(Gs - Gr).max() <= tol_G(Gr)


@pytest.mark.parametrize("N,L", [(16, 1), (32, 2), (9, 2), (16, 4), (30, 6), (4, 8)])
def test_small_sizes_one_wave_per_batch_and_the_hand_over_of_sub_stepped_series(g, ref, N, L, monkeypatch):
    """N <= 32 (Hermitian operators, L <= 8): the derivative overlaps come from deriv3_kernel unless a batch needs a
    sub-stepped series (||H|| dt above the threshold) -- then deriv_flag_kernel has counted it, deriv3_kernel leaves at once
    and deriv_kernel, launched behind it, does every cell: bit-identical to GRAPE_DERIV3=0.  Without such a batch the two
    kernels agree to rounding; either way the result matches the C restatement."""
    from grape_jl_amd import synth
    N_T, K = 75, 5
    pr = synth.make_problem(N, L, N_T, K, seed=4100 + N)
    for big in (False, True):
        dts = np.full(N_T, 0.8)
        if big:
            dts[[7, 40]] = 9.0                            # ||H|| dt about 9: sub-steps
        tl = np.concatenate([[0.0], np.cumsum(dts)])
        args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"])
        res = {}
        for name, env in (("d3", {}), ("old", {"GRAPE_DERIV3": "0"})):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            with g.GrapeHip(*args) as h:
                J, G, tau = h.eval(pr["pulsevals"])
                res[name] = (J, G.copy(), h.work()["deriv_orders"])
            for k in env:
                monkeypatch.delenv(k)
        assert res["d3"][0] == res["old"][0]
        if big:
            assert np.array_equal(res["d3"][1], res["old"][1]) and res["d3"][2] == res["old"][2]
        else:
            assert np.abs(res["d3"][1] - res["old"][1]).max() <= 1e-13 * max(np.abs(res["old"][1]).max(), 1e-3)
        Jr, Gr, taur = ref.evaluate(*args[:3], pr["pulsevals"], *args[3:])
        assert abs(res["d3"][0] - Jr) <= TOL_J and np.abs(res["d3"][1] - Gr).max() <= tol_G(Gr)


@pytest.mark.parametrize("N,L,N_T,K", [(64, 2, 100, 3), (48, 1, 75, 5), (44, 2, 33, 2)])
def test_general_drift_with_hermitian_controls_one_wave_per_batch(g, ref, N, L, N_T, K, monkeypatch):
    """A non-Hermitian drift H0_k (effective Hamiltonian with decay) beside Hermitian control operators: deriv3_kernel keeps
    ALL tiles of H0_k in LDS, reads them directly in pass 1 and as the adjoint -- every tile transposed, conjugated through
    the negation bit of the matrix instruction -- in pass 2 (grape_deriv3.hip.h, H0G).  Against deriv2_kernel
    (GRAPE_DERIV3=0) and the C restatement."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=5100 + N, hermitian=False)
    tl = pr["tlist"] * 0.7
    args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"])
    res = {}
    for name, env in (("d3", {}), ("d2", {"GRAPE_DERIV3": "0"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with g.GrapeHip(*args) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            res[name] = (J, G.copy(), h.work()["deriv_orders"])
        for k in env:
            monkeypatch.delenv(k)
    assert res["d3"][0] == res["d2"][0]
    if N > 48:   # four tiles per side: the streamed all-tiles assembly kernel (asm/gen_d3s.py GenD3G) -- the four batches of a
                 # workgroup stop together, never earlier than each alone
        assert 0 < res["d2"][2] <= res["d3"][2] <= res["d2"][2] + K * N_T
    else:
        assert res["d3"][2] == res["d2"][2] > 0
    assert np.abs(res["d3"][1] - res["d2"][1]).max() <= 1e-13 * max(np.abs(res["d2"][1]).max(), 1e-3)
    ns = 12
    xs = pr["pulsevals"].reshape(L, N_T)[:, :ns].reshape(-1)
    with g.GrapeHip(pr["H0"], pr["Hc"], tl[: ns + 1], pr["psi0"], pr["target"], pr["weights"]) as hs:
        Js, Gs, taus = hs.eval(xs)
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], tl[: ns + 1], xs, pr["psi0"], pr["target"], pr["weights"],
                                gradient_method=ref.TAYLOR)
    assert abs(Js - Jr) <= TOL_J * max(1.0, abs(Jr)) and np.abs(taus - taur).max() <= TOL_TAU * max(1.0, np.abs(taur).max())
    assert np.abs(Gs - Gr).max() <= tol_G(Gr)


def test_taylor_route_honours_max_order_beyond_the_parked_terms(g, ref):
    """gradient_method = :taylor, N <= 32, a step large enough that the recursion of taylor_grad_step! needs more than the 64
    terms deriv3_kernel parks but fewer than taylor_grad_max_order (reference default 100, src/optimize.jl:914): the
    one-wave-per-batch kernel asks for deriv_kernel, which honours any order, instead of reporting non-convergence (round-3
    advisor finding).  The plain series loses digits like e^(||H|| dt) -- in the restatement too: compared at 1e-5."""
    from grape_jl_amd import synth
    pr = synth.make_problem(8, 1, 3, 2, seed=90)
    tl = pr["tlist"] * 19.5                              # ||H|| dt ~ 20: ~70 terms
    args = (pr["H0"], pr["Hc"], tl, pr["psi0"], pr["target"], pr["weights"])
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                gradient_method=ref.TAYLOR)
    with g.GrapeHip(*args, gradient_method=1) as h:
        J, G, tau = h.eval(pr["pulsevals"])
        orders = h.work()["deriv_orders"] / h.work()["cells"]
    assert orders > 64
    assert abs(J - Jr) <= 1e-9 and np.abs(G - Gr).max() <= 1e-5 * max(np.abs(Gr).max(), 1e-3)
    with g.GrapeHip(*args, gradient_method=1, taylor_max_order=40) as h:     # ... and the reference's error when it is not enough
        with pytest.raises(g.GrapeHipError):
            h.eval(pr["pulsevals"])
