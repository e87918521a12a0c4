"""The pre-launch certificate of the four-product assembly cell on the device (needs an MI355X): t16_plan_kernel certifies
cells from the trace tables of their generator class (grape_cert.hip.h) and such cells skip the in-cell spectral bound
(asm/gen_t16.py).  With the certificate on (default) and off (GRAPE_EXPM_CERT=0, read in grape_create) every result must be
the same bits; grape_get_work[19] counts the certified cells.  All cases: N = 64, K = 3, N_T = 24."""
import os

import numpy as np
import pytest

from test_cert_table import evaluate

pytestmark = pytest.mark.gpu

N, K, N_T = 64, 3, 24
THETA = 1.36


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    assert os.path.exists(mod.library_path()), "HIP extension missing: the product path has no fallback"
    return mod


def run(g, pr, cert, **kw):
    old = os.environ.get("GRAPE_EXPM_CERT")
    os.environ["GRAPE_EXPM_CERT"] = "1" if cert else "0"
    try:
        with g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], **kw) as h:
            J, G, tau = h.eval(pr["pulsevals"])
            w = h.work()
            U = np.stack([h.propagator(k, n) for k in range(K) for n in range(N_T)])
            return dict(J=J, G=G.copy(), tau=tau.copy(), U=U, fw=h.storage(0), bw=h.storage(1), work=w, table=h.cert_table())
    finally:
        if old is None:
            os.environ.pop("GRAPE_EXPM_CERT", None)
        else:
            os.environ["GRAPE_EXPM_CERT"] = old


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def assert_same_bits(a, b):
    assert a["J"] == b["J"]
    for name in ("G", "tau", "U", "fw", "bw"):
        assert np.array_equal(bits(a[name]), bits(b[name])), name
    for name in ("t16_cells", "t18_cells", "t18_squarings", "t18_mfma_flop", "deriv_orders", "walk_steps", "flop_expm", "squarings"):
        assert a["work"][name] == b["work"][name], name


def handed_over(r):
    return r["work"]["t18_cells"] - r["work"]["t16_cells"]


def moments(pr, k, n, per_traj=False, shape=None):
    L = pr["pulsevals"].size // N_T
    e = pr["pulsevals"].reshape(L, N_T)[:, n] * (1.0 if shape is None else shape[:, n])
    Hc = pr["Hc"][k] if per_traj else pr["Hc"]
    lam = np.linalg.eigvalsh(pr["H0"][k] + sum(e[l] * Hc[l] for l in range(L)))
    return e, np.sum(lam ** 8), np.sum(lam ** 6)


def test_benchmark_like_cells_are_all_certified_and_nothing_changes(g):
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, N_T, K, seed=3)
    # (on the CPU: every cell is inside the certificate with margin -- the bound m8^(1/8) of such cells is 1.17 .. 1.29)
    for k in range(K):
        for n in range(N_T):
            assert moments(pr, k, n)[1] ** 0.125 <= 0.97 * THETA
    on, off = run(g, pr, True), run(g, pr, False)
    assert_same_bits(on, off)
    assert on["work"]["t16_certified"] == K * N_T and off["work"]["t16_certified"] == 0
    assert on["work"]["asm_kernel"] == 1 and off["work"]["asm_kernel"] == 1
    assert on["work"]["t16_cells"] == K * N_T
    assert off["table"][0].size == 0            # no tables without the certificate


@pytest.mark.parametrize("L", (1, 2, 3))
def test_device_tables_against_the_moments_of_the_eigenvalues(g, L):
    from grape_jl_amd import synth
    pr = synth.make_problem(N, L, N_T, K, seed=40 + L)
    on = run(g, pr, True)
    t8, t6, ex = on["table"]
    n8 = {1: 9, 2: 45, 3: 165}[L]
    assert t8.shape == (K, n8) and ex.shape[1] == L
    worst = 0.0
    for k in range(K):
        for n in range(N_T):
            e, m8, m6 = moments(pr, k, n)
            p8, S8 = evaluate(t8[k], ex[:n8], e)
            p6, _ = evaluate(t6[k], ex[n8:], e)
            assert abs(p8 - m8) <= 1e-12 * m8 and abs(p6 - m6) <= 1e-12 * m6, (k, n, p8 / m8 - 1, p6 / m6 - 1)
            assert abs(p8 - m8) <= 2.0 ** -30 * S8
            worst = max(worst, abs(p8 / m8 - 1), abs(p6 / m6 - 1))
    print("worst relative error of the device tables: %.2e" % worst)
    assert on["work"]["t16_certified"] == K * N_T


def test_long_steps_are_certified_with_their_planned_squarings(g):
    """dt = 1.5: the plan gives the cells squarings, and the certificate is taken for A / 2^s"""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, N_T, K, seed=3)
    pr["tlist"] = pr["tlist"] * 1.5
    on, off = run(g, pr, True), run(g, pr, False)
    assert_same_bits(on, off)
    assert on["work"]["t18_squarings"] > 0
    assert on["work"]["t16_certified"] > 0 and off["work"]["t16_certified"] == 0
    assert handed_over(on) == handed_over(off)


def test_a_cell_beyond_the_bound_at_the_end_of_the_trajectories(g):
    """one pulse value of 4 pi at n = N_T - 1: the last cell of every trajectory is beyond what three squarings bring into range
    (on the CPU: m8^(1/8) / 8 > 1.36), so it is neither certified nor passed by the cell -- the descending walks must not enter
    their trajectories through it -- and goes to the five-product launch; every other cell is certified"""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, N_T, K, seed=3)
    pr["pulsevals"][N_T - 1] = 4.0 * np.pi
    for k in range(K):
        assert moments(pr, k, N_T - 1)[1] ** 0.125 / 8.0 > 1.05 * THETA
    on, off = run(g, pr, True), run(g, pr, False)
    assert_same_bits(on, off)
    assert 0 < on["work"]["t16_certified"] < K * N_T
    assert on["work"]["t16_certified"] == K * (N_T - 1)
    assert handed_over(on) == handed_over(off) == K


def test_cells_only_the_one_norm_passes_are_left_to_the_cell(g):
    """controls C1 = P + Q, C2 = P - Q with equal pulse values on a weak drift: H = H0 + 2 e P, P = diag(1, -1, 1, -1, 0, ..).
    Four eigenvalues of 1.2: m8 = 4 * 1.2^8 is beyond theta^8 (the Schatten bound fails, in the cell and in the certificate)
    while ||A^2||_1 = 1.44 + (drift) is inside theta^2 -- the cell's 1-norm alternative passes it.  The plan's estimate
    takes the controls for the full-rank operators they are and tries the route.  Nothing is certified, nothing changes."""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, N_T, K, seed=8)
    P = np.zeros((N, N), complex)
    P[range(4), range(4)] = [1.0, -1.0, 1.0, -1.0]
    Q = np.zeros((N, N), complex)
    Q[4:, 4:] = 0.5 * synth.gue(123, N - 4)
    pr["Hc"] = np.stack([P + Q, P - Q])
    pr["H0"] = np.stack([0.01 * synth.gue(70 + k, N) for k in range(K)])
    pr["pulsevals"] = np.full(2 * N_T, 0.6)
    for k in range(K):
        e, m8, m6 = moments(pr, k, 0)
        H = pr["H0"][k] + 0.6 * (pr["Hc"][0] + pr["Hc"][1])
        A2 = H @ H
        n2 = (np.abs(A2.real) + np.abs(A2.imag)).sum(axis=0).max()
        assert m8 > 1.3 * THETA ** 8 and n2 < 0.9 * THETA ** 2 and m6 > 0      # the reference inequalities decide, with margin
    on, off = run(g, pr, True), run(g, pr, False)
    assert_same_bits(on, off)
    assert on["work"]["t16_certified"] == 0
    assert on["work"]["t16_cells"] == K * N_T and handed_over(on) == 0        # the cell passed them all (1-norm)


def test_control_operators_per_trajectory(g):
    """the variant that fetches the control operators of its trajectory (expm_t16p_asm) inherits the certified path; the tables
    are built from every trajectory's own operators"""
    from grape_jl_amd import synth
    pr = synth.make_problem(N, 2, N_T, K, seed=5)
    rng = np.random.default_rng(4)
    pr["Hc"] = np.stack([pr["Hc"] * (1.0 + 0.1 * rng.random()) for _ in range(K)])
    on, off = run(g, pr, True), run(g, pr, False)
    assert_same_bits(on, off)
    assert on["work"]["asm_kernel"] == 3
    assert on["work"]["t16_certified"] == K * N_T and off["work"]["t16_certified"] == 0
    t8, t6, ex = on["table"]
    for k in range(K):
        e, m8, m6 = moments(pr, k, 7, per_traj=True)
        p8, S8 = evaluate(t8[k], ex[:45], e)
        assert abs(p8 - m8) <= 1e-12 * m8 and abs(p8 - m8) <= 2.0 ** -30 * S8
