"""The degree-15 derivative series on the device (needs an MI355X): cells the plan certifies for a spectral radius of
at most 1.11 from three trace moments (t16_seg_certified; tables of grape_create, GRAPE_DERIV_SEG=0: none) take the
degree-15 polynomial of grape_econ_coeffs.h in the derivative kernels; a batch of 16 cells runs the largest degree of its
cells.  grape_get_work[4] (deriv_orders) says what ran, [20] (seg_certified) how many cells qualified, and
grape_get_seg_table hands out the tables the plan reads.  Every expectation
about which cells qualify is established on the CPU from the eigenvalues (tests/seg_cert_reference.py)."""
import os

import numpy as np
import pytest

import seg_cert_reference as sc

pytestmark = pytest.mark.gpu

TH = sc.THETA15
T16_THETA = 1.36
ENVS = ("GRAPE_DERIV_SEG", "GRAPE_EXPM_CERT", "GRAPE_DERIV3_ASM")


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


def run(g, pr, seg=True, cert=True, asm=True):
    old = {name: os.environ.get(name) for name in ENVS}
    os.environ.update(GRAPE_DERIV_SEG="1" if seg else "0", GRAPE_EXPM_CERT="1" if cert else "0", GRAPE_DERIV3_ASM="1" if asm else "0")
    try:
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"]) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            J2, G2, _ = h.eval(pr["pulsevals"])
            assert J2 == J and np.array_equal(G, G2)         # repeatable bit for bit
            return dict(J=J, G=G.copy(), tau=tau.copy(), fw=h.storage(0), bw=h.storage(1), work=h.work(), table=h.cert_table(),
                        seg=h.seg_table())
    finally:
        for name, val in old.items():
            if val is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = val


def bounds(pr):
    """[K][N_T] three-moment bound, m8^(1/8) and spectral radius of every cell, from the eigenvalues"""
    K, N_T = pr["K"], pr["N_T"]
    b, m8, rho = np.zeros((K, N_T)), np.zeros((K, N_T)), np.zeros((K, N_T))
    for k in range(K):
        for n in range(N_T):
            lam = sc.cell_spectrum(pr, k, n)
            b[k, n], m8[k, n], rho[k, n] = sc.three_moment_bound(lam), sc.moments(lam)[1] ** 0.125, np.abs(lam).max()
    return b, m8, rho


def assert_oracle(ref, pr, r):
    Jr, Gr, taur = ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"],
                                gradient_method=ref.GRADGEN)
    assert abs(r["J"] - Jr) <= 1e-12 and np.abs(r["tau"] - taur).max() <= 1e-12
    assert np.abs(r["G"] - Gr).max() <= 1e-10 * max(np.abs(Gr).max(), 1e-3)


def assert_close(a, b):
    """two series for the same derivative: the Taylor sum's numbers to 1e-13 (tests/test_gpu_asm.py)"""
    assert a["J"] == b["J"] and np.array_equal(a["tau"], b["tau"])
    gs = max(np.abs(b["G"]).max(), 1e-3)
    assert np.abs(a["G"] - b["G"]).max() <= 1e-13 * gs, np.abs(a["G"] - b["G"]).max() / gs


def assert_same_bits(a, b):
    assert a["J"] == b["J"]
    for name in ("G", "tau", "fw", "bw"):
        assert np.array_equal(np.ascontiguousarray(a[name]).view(np.uint64), np.ascontiguousarray(b[name]).view(np.uint64)), name
    for name in ("deriv_orders", "seg_certified", "t16_cells", "t18_cells", "t18_squarings"):
        assert a["work"][name] == b["work"][name], name


def problem(N, seed, L=2, K=2, N_T=40):
    from grape_jl_amd import synth
    return synth.make_problem(N, L, N_T, K, seed=seed)


@pytest.mark.parametrize("N,seed", [(64, 2), (49, 1)])
def test_certifiable_cells_run_degree_15(g, ref, N, seed):
    """two full batches and a half one per trajectory, every cell certifiable with margin"""
    pr = problem(N, seed)
    K, N_T = pr["K"], pr["N_T"]
    assert bounds(pr)[0].max() <= 0.995 * TH
    on, off = run(g, pr), run(g, pr, seg=False)
    assert on["work"]["deriv_orders"] == 15 * K * N_T and off["work"]["deriv_orders"] == 16 * K * N_T
    assert on["work"]["seg_certified"] == K * N_T and off["work"]["seg_certified"] == 0
    assert on["work"]["asm_kernel"] == 1 and on["work"]["asm_deriv_kernel"] == 1
    assert_oracle(ref, pr, on)
    assert_close(on, off)
    # the expm certificate shares its tr H^8 table with the segment tables or leaves them their own: the same bits
    nocert = run(g, pr, cert=False)
    assert_same_bits(on, nocert)
    assert nocert["table"][0].size == 0 and nocert["work"]["t16_certified"] == 0 and on["work"]["t16_certified"] == K * N_T
    assert_same_bits(off, run(g, pr, seg=False, cert=False))


@pytest.mark.parametrize("N,L,per_traj", [(64, 2, False), (49, 2, False), (64, 1, False), (64, 2, True)])
def test_device_tables_against_the_moments_of_the_eigenvalues(g, N, L, per_traj):
    """what grape_create built and the plan reads (grape_get_seg_table): t4, t8, t12 of every class and their exponent words
    reproduce the moments of the eigenvalues to 1e-12 relative and far inside the guard 2^-30 S of the device's test -- with
    the certificate's t8 (default) and with the segment tables' own copy (GRAPE_EXPM_CERT=0), which are the same bits"""
    pr = problem(N, 30 + N + L, L=L, N_T=12)
    K, N_T = pr["K"], pr["N_T"]
    if per_traj:
        pr["Hc"] = np.stack([pr["Hc"] * f for f in (1.0, 0.9)])
    on, own = run(g, pr), run(g, pr, cert=False)
    n4, n8, n12 = (15, 45, 91) if L == 2 else (5, 9, 13)
    worst = 0.0
    for r in (on, own):
        t4, t8, t12, ex = r["seg"]
        assert t4.shape == (K, n4) and t8.shape == (K, n8) and t12.shape == (K, n12) and ex.shape == (n4 + n8 + n12, L)
        e4, e8, e12 = ex[:n4], ex[n4:n4 + n8], ex[n4 + n8:]
        for x, d in ((e4, 4), (e8, 8), (e12, 12)):
            assert (x.sum(axis=1) <= d).all() and len({tuple(row) for row in x}) == len(x)      # every monomial once
        for k in range(K):
            for n in range(N_T):
                H, _, e = sc.cell_generator(pr, k, n)
                for t, x, m in zip((t4[k], t8[k], t12[k]), (e4, e8, e12), sc.moments(np.linalg.eigvalsh(H))):
                    p, S = sc.poly(t, x, e)
                    assert abs(p - m) <= 1e-12 * m, (k, n, len(t), p / m - 1)
                    assert abs(p - m) <= sc.G * S
                    worst = max(worst, abs(p / m - 1))
    print("worst relative error of the device's segment tables: %.2e" % worst)
    for a, b in zip(on["seg"], own["seg"]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    assert np.array_equal(on["seg"][1], on["table"][0]) and own["table"][0].size == 0          # the shared t8 is the certificate's
    assert all(x.size == 0 for x in run(g, pr, seg=False)["seg"][:3])                            # no tables without the switch


def stretched(pr, n, dt):
    out = dict(pr)
    d = np.diff(pr["tlist"])
    d[n] = dt
    out["tlist"] = np.concatenate([[0.0], np.cumsum(d)])
    return out


@pytest.mark.parametrize("N,seed", [(64, 2), (49, 1)])
def test_one_cell_beyond_the_segment_costs_its_batch_one_order(g, ref, N, seed):
    pr0 = problem(N, seed)
    K, N_T, n = pr0["K"], pr0["N_T"], 20
    b0 = bounds(pr0)[0]
    pr = stretched(pr0, n, 1.012 * TH / b0[:, n].min())
    b, m8, _ = bounds(pr)
    assert (b[:, n] > 1.01 * TH).all() and (m8[:, n] <= 0.97 * T16_THETA).all()
    assert np.delete(b, n, axis=1).max() <= 0.995 * TH
    on, off = run(g, pr), run(g, pr, seg=False)
    assert on["work"]["deriv_orders"] == 15 * K * (N_T - 16) + 16 * K * 16          # only the batch of cell n runs degree 16
    assert on["work"]["seg_certified"] == K * (N_T - 1)
    assert off["work"]["deriv_orders"] == 16 * K * N_T
    assert_oracle(ref, pr, on)
    assert_close(on, off)


def test_a_cell_with_a_planned_squaring_keeps_degree_21(g, ref):
    pr0 = problem(64, 2)
    K, N_T, n = pr0["K"], pr0["N_T"], 20
    pr = stretched(pr0, n, 1.5)
    b, m8, rho = bounds(pr)
    assert (m8[:, n] > T16_THETA).all() and (m8[:, n] / 2 <= 0.97 * T16_THETA).all()     # out of the four products' range unless halved
    on, off = run(g, pr), run(g, pr, seg=False)
    assert on["work"]["t18_squarings"] == K                                              # one squaring, in that cell alone
    assert on["work"]["seg_certified"] == K * (N_T - 1)
    assert on["work"]["deriv_orders"] == 15 * K * (N_T - 16) + 21 * K * 16
    assert off["work"]["deriv_orders"] == 16 * K * (N_T - 16) + 21 * K * 16
    assert_oracle(ref, pr, on)
    assert_close(on, off)


def test_one_control(g, ref):
    pr = problem(64, 1, L=1, N_T=24)
    K, N_T = pr["K"], pr["N_T"]
    assert bounds(pr)[0].max() <= 0.995 * TH
    on, off = run(g, pr), run(g, pr, seg=False)
    assert on["work"]["deriv_orders"] == 15 * K * N_T and on["work"]["seg_certified"] == K * N_T
    assert_oracle(ref, pr, on)
    assert_close(on, off)


def test_control_operators_per_trajectory(g, ref):
    """expm_t16p_asm: every trajectory is a generator class of its own, with its own tables"""
    pr = problem(64, 2, N_T=24)
    K, N_T = pr["K"], pr["N_T"]
    pr["Hc"] = np.stack([pr["Hc"] * f for f in (1.0, 0.9)])
    b = bounds(pr)[0]
    assert b.max() <= 0.995 * TH
    on, off = run(g, pr), run(g, pr, seg=False)
    assert on["work"]["asm_kernel"] == 3
    assert on["work"]["deriv_orders"] == 15 * K * N_T and on["work"]["seg_certified"] == K * N_T
    assert_oracle(ref, pr, on)
    assert_close(on, off)


def test_compiled_twin_reads_the_same_tables(g):
    """GRAPE_DERIV3_ASM=0: deriv3_kernel<4, L> takes the degrees and the scalars of deriv3_asm"""
    pr = problem(64, 2)
    a, c = run(g, pr), run(g, pr, asm=False)
    assert a["work"]["asm_deriv_kernel"] == 1 and c["work"]["asm_deriv_kernel"] == 0
    assert c["work"]["deriv_orders"] == a["work"]["deriv_orders"] == 15 * pr["K"] * pr["N_T"]
    assert_close(c, a)


def test_two_tiles_per_side_are_unaffected(g):
    """N = 32 takes the compiled four-product kernel: no tables, no plan words -- the switch changes nothing"""
    pr = problem(32, 5)
    on, off = run(g, pr), run(g, pr, seg=False)
    assert on["work"]["seg_certified"] == 0 and on["work"]["asm_kernel"] == 0
    assert_same_bits(on, off)
