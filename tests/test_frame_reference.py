"""The reference of the frame tests (tests/frame_reference.py) proved on the CPU: against the numpy oracle with callbacks,
against the C restatement (D, evaluate_chi), against central differences of its own J in the pulses and in the time steps, by
``skewed()`` evaluated directly, and by the shared comparison refusing five deliberately wrong references.  No GPU, nothing of
the product path."""
import numpy as np
import pytest

import frame_reference as fr

MODES = "abcde"
GOT_KEYS = ("J", "Jb", "tau", "G", "tau_grads", "dJdt", "dJdt_prop", "psiT", "fw", "bw")


def as_got(res, mode, k=0, n=1):
    got = {key: res[key] for key in GOT_KEYS}
    got.update(bwT=res["bw"][:, -1], U=res["U"][k, n], Ukn=(k, n))
    if mode in "cd":       # the caller's J_T: J is not the library's to know
        del got["J"]
    return got


@pytest.fixture(scope="module")
def small():
    """N = 6, general generators, K = 3, L = 2, N_T = 4, non-uniform grid, weights, shape; J_T_ss"""
    pr = fr.make_twin(6, 2, 3, 4, seed=6006, kind="general")
    prs, want = fr.all_modes(pr, 1, seed=6006, per_traj_D=True)
    return pr, prs, want


def test_signals_are_order_one(small):
    _, _, want = small
    fr.assert_order_one(want["a"])
    fr.assert_order_one(want["b"])
    fr.assert_order_one(want["e"], running_cost=False)


@pytest.mark.parametrize("kind", ["herm", "general"])
@pytest.mark.parametrize("functional", [0, 1, 2])
def test_reference_against_the_numpy_oracle_with_callbacks(kind, functional):
    """grape_oracle.evaluate_gradient with g_b / xi callbacks and with D, with a shape and a non-uniform grid: J, tau, G, the
    stored forward states, the normalised backward states, rho and every tau_grads entry"""
    import grape_oracle as go
    pr = fr.make_twin(4, 2, 2, 5, seed=4100 + functional, kind=kind)
    prs, want = fr.all_modes(pr, functional, seed=41)
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["pulsevals"], pr["psi0"], pr["target"], pr["weights"])
    for mode, kw in (("a", dict(D=prs["a"]["D"], lambda_b=prs["a"]["lambda_b"])),
                     ("b", dict(g_b=prs["b"]["g_b"], xi=prs["b"]["xi"], lambda_b=prs["b"]["lambda_b"])), ("e", {})):
        J, G, tau, parts = go.evaluate_gradient(*args, functional=functional, shape=pr["shape"], return_parts=True, **kw)
        w = want[mode]
        got = dict(J=J, G=G, tau=tau, fw=parts["storage"], bw=parts["chi"], tau_grads=np.swapaxes(parts["tau_grads"], 1, 2))
        fr.assert_agrees(got, w, f"oracle {kind} f{functional} ({mode})")
        assert np.abs(parts["rho"] - w["rho"]).max() <= 1e-13
        assert np.abs(np.swapaxes(parts["tau_grads"], 1, 2) - w["tau_grads"]).max() <= 1e-12


@pytest.mark.parametrize("kind", ["herm", "general"])
def test_reference_against_the_c_restatement(ref, kind):
    """oracle/grape_ref.c: the built-in running cost (shared and per-trajectory D) and a caller's chi with it (no shape: the
    restatement has none)"""
    pr = fr.make_twin(5, 2, 3, 4, seed=5200, kind=kind)
    pr["shape"] = None
    fr.order_one_targets(pr)
    x = pr["pulsevals"]
    args = (pr["H0"], pr["Hc"], pr["tlist"], x, pr["psi0"], pr["target"])
    ctx = fr.propagate(pr, x)
    for per_traj in (False, True):
        D = fr.penalty(5, 52, 3 if per_traj else None)
        for functional in (0, 1, 2):
            want = fr.evaluate(dict(pr, D=D, lambda_b=0.3), x, functional, ctx=ctx)
            J, G, tau, parts = ref.evaluate(*args, pr["weights"], functional=functional, want_parts=True, D=D, lambda_b=0.3)
            fr.assert_agrees(dict(J=J, G=G, tau=tau, psiT=parts["psiT"], tau_grads=parts["tau_grads"]), want, f"C {kind} f{functional}")
        chi = fr.observable_chi(ctx["fw"][:, -1], pr["weights"], 52)
        want = fr.evaluate(dict(pr, D=D, lambda_b=0.3, chi=chi), x, ctx=ctx)
        G, tau, psiT, tg = ref.evaluate_chi(*args, chi, weights=pr["weights"], D=D, lambda_b=0.3)
        fr.assert_agrees(dict(G=G, tau=tau, psiT=psiT, tau_grads=tg), want, f"C {kind} chi")
        want = fr.evaluate(dict(pr, chi=chi), x, ctx=ctx)
        G, *_ = ref.evaluate_chi(*args, chi, weights=pr["weights"])
        fr.assert_agrees(dict(G=G), want, f"C {kind} chi alone")


# Deviation of G and dJdt from central differences of the reference's own J (step 1e-5, J = O(1): rounding 1e-16 / 1e-5 plus the
# h^2 term), relative to the sup norm: measured <= 4e-10 over the cases below.  The bound is 1e-7, the figure the suite uses
# for central differences everywhere (tests/test_gpu_time_grid.py, tests/test_gpu_boundary.py).
FD_BOUND = 1e-7


@pytest.mark.parametrize("mode", ["a", "b", "e"])
def test_gradient_against_central_differences_of_J(small, mode):
    pr, prs, want = small
    p, x, h = prs[mode], pr["pulsevals"], 1e-5
    fd = np.empty_like(x)
    for i in range(len(x)):
        d = np.zeros_like(x)
        d[i] = h
        fd[i] = (fr.evaluate(p, x + d, 1)["J"] - fr.evaluate(p, x - d, 1)["J"]) / (2 * h)
    rel = np.abs(fd - want[mode]["G"]).max() / np.abs(want[mode]["G"]).max()
    print(dict(mode=mode, fd_deviation_rel=rel, bound=FD_BOUND))
    assert rel <= FD_BOUND


@pytest.mark.parametrize("mode", ["a", "b", "e"])
def test_time_gradient_against_central_differences_in_dt(small, mode):
    """propagation part plus weight term: dt_n grows, every later grid point moves along (pulse and shape values fixed)"""
    pr, prs, want = small
    p, x, tl = prs[mode], pr["pulsevals"], np.asarray(pr["tlist"])
    fd = np.empty(len(tl) - 1)
    for n in range(len(fd)):
        h = 1e-5 * (tl[n + 1] - tl[n])
        Jpm = []
        for sgn in (1, -1):
            t2 = tl.copy()
            t2[n + 1:] += sgn * h
            Jpm.append(fr.evaluate(dict(p, tlist=t2), x, 1)["J"])
        fd[n] = (Jpm[0] - Jpm[1]) / (2 * h)
    rel = np.abs(fd - want[mode]["dJdt"]).max() / np.abs(want[mode]["dJdt"]).max()
    print(dict(mode=mode, fd_deviation_rel=rel, bound=FD_BOUND))
    assert rel <= FD_BOUND
    if mode == "e":
        assert np.all(want[mode]["dJdt_weight"] == 0.0)
    else:
        assert np.abs(want[mode]["dJdt_weight"]).max() >= 1e-3    # the weight term is part of what the differences confirm


@pytest.mark.parametrize("mode", list(MODES))
def test_skewed_problem_gives_the_mapped_values_of_the_twin(small, mode):
    """skewed() evaluated directly by the reference (no balancing anywhere): J, J_b, tau, G, dJdt are the twin's, the states
    and the propagator map back to the twin's"""
    pr, prs, want = small
    e = fr.skew_exponents(6, 66)
    sk = fr.skewed(prs[mode], e)
    S = 2.0 ** e
    assert np.array_equal(sk["H0"], S[:, None] * pr["H0"] / S[None, :]) and np.array_equal(sk["psi0"], pr["psi0"] * S)
    res = fr.evaluate(sk, pr["pulsevals"], 1)
    fr.assert_agrees(as_got(res, mode), want[mode], f"skewed ({mode})", e=e)
    # and the frame is not trivial: unmapped, the states are refused
    with pytest.raises(AssertionError):
        fr.assert_agrees(dict(fw=res["fw"]), want[mode], "unmapped")


@pytest.mark.parametrize("wrong", fr.WRONG)
def test_the_comparison_refuses_wrong_references(small, wrong):
    """every deliberate mistake moves a compared quantity by far more than its bar"""
    pr, prs, want = small
    e = fr.skew_exponents(6, 66)
    x = pr["pulsevals"]
    if wrong == "dpen_similarity":
        mode, bad = "a", fr.evaluate(fr.skewed(prs["a"], e, wrong=wrong), x, 1)
    elif wrong == "chi_unscaled":
        mode, bad = "c", fr.evaluate(fr.skewed(prs["c"], e, wrong=wrong), x, 1)
    else:
        mode, bad = "a", fr.evaluate(prs["a"], x, 1, wrong=wrong)
        e = None
    fr.assert_agrees(as_got(want[mode], mode), want[mode], "right")
    for key in ("G", "dJdt"):
        with pytest.raises(AssertionError):
            fr.assert_agrees({key: bad[key]}, want[mode], f"{wrong}: {key}", e=e)
    if wrong in ("trapezoid_end", "dpen_similarity"):
        with pytest.raises(AssertionError):
            fr.assert_agrees(dict(Jb=bad["Jb"]), want[mode], f"{wrong}: Jb", e=e)
    if wrong in ("drop_xi_T", "chi_unscaled"):
        with pytest.raises(AssertionError):
            fr.assert_agrees(dict(bwT=bad["bw"][:, -1]), want[mode], f"{wrong}: chi(T)", e=e)
    # the squared cost through xi sees the three mistakes of the recursion as well
    if e is None:
        badb = fr.evaluate(prs["b"], x, 1, wrong=wrong)
        with pytest.raises(AssertionError):
            fr.assert_agrees(dict(G=badb["G"]), want["b"], f"{wrong}: G (b)")
