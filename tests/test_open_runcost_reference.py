"""tests/open_runcost_reference.py is what tests/test_gpu_open_runcost.py measures the running-cost kernels with, so it is
proved here first, without a GPU:
  - against oracle/grape_oracle.py evaluate_gradient on the vectorised problem (open_helpers.vectorised) with the callbacks
    g_b = Re vdot(vec D^dagger, psi) and xi = -vec(D^dagger) / 2;
  - double against x87 long double, and a nonlinear caller cost (g_b = -tr rho^dagger rho, xi = rho) against central
    differences of the reference's own J; the bound is 1e-14, a hundredth of the GPU tolerances;
  - the shared comparison open_runcost_reference.assert_runcost_agrees must REFUSE seven deliberately wrong references.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
import open_runcost_reference as rcf  # noqa: E402
from test_open_reference import _problem  # noqa: E402

BOUND = 1e-14


def _worst(a, b, keys):
    fig = {key: float(np.abs(np.asarray(a[key]) - np.asarray(b[key])).max()) for key in keys}
    print(fig)
    return max(fig.values())


def _oracle(pr, functional, D, lambda_b):
    """grape_oracle.evaluate_gradient on the vectorised problem: dict(J, J_b, G, tau, rhoT, tau_grads)"""
    import grape_oracle as go
    v = oh.vectorised(pr)
    K, d = pr["H0"].shape[0], pr["H0"].shape[1]
    Dd = np.conj(np.swapaxes(np.asarray(D), -1, -2))
    xi_vec = oh.vec(Dd)                                       # [d*d] or [K, d*d]
    of = (lambda k: xi_vec) if xi_vec.ndim == 1 else (lambda k: xi_vec[k])
    kw = {} if D is None or lambda_b == 0.0 else dict(g_b=lambda psi, k, n: float(np.real(np.vdot(of(k), psi))),
                                                       xi=lambda psi, k, n: -of(k) / 2.0, lambda_b=lambda_b)
    J, G, tau, parts = go.evaluate_gradient(v["H0"], v["Hc"], pr["tlist"], pr["pulsevals"], v["psi0"], v["target"], pr["weights"],
                                            functional=functional, shape=pr["shape"], return_parts=True, **kw)
    out = dict(J=J, G=G, tau=tau, rhoT=np.swapaxes(parts["storage"][:, -1].reshape(K, d, d), -1, -2),
               tau_grads=np.transpose(parts["tau_grads"], (0, 2, 1)))
    if kw:
        out["J_b"] = sum(go.J_b_trajectory(None, parts["storage"][k], pr["tlist"], kw["g_b"], k) for k in range(K))
    return out


ROWS = [dict(d=2, J=0, L=3, functional=2), dict(d=2, J=3, L=1, functional=1, K=3, d_per_traj=True),
        dict(d=4, J=3, L=1, functional=0), dict(d=4, J=0, L=3, functional=2, hc_per_traj=True, d_per_traj=True),
        dict(d=5, J=3, L=3, functional=1, cops_per_traj=True, K=3), dict(d=5, J=0, L=1, functional=0, d_per_traj=True),
        dict(d=5, J=3, L=3, functional=2, chi=True)]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "-".join(f"{k}{v}" for k, v in r.items()))
def test_against_the_oracle_on_the_vectorised_problem(row):
    """weights, a shape and a non-uniform grid in every row (test_open_reference._problem)"""
    row = dict(row)
    functional, per_traj, with_chi = row.pop("functional"), row.pop("d_per_traj", False), row.pop("chi", False)
    pr = _problem(N_T=3, **row)
    K, d = pr["H0"].shape[0], pr["H0"].shape[1]
    D = rcf.hermitian_D(77 + d, d, K if per_traj else None)
    lam = 0.75
    want, want_T = _oracle(pr, functional, D, lam), _oracle(pr, functional, D, 0.0)
    chi = (pr["weights"] / (2.0 * K))[:, None, None] * pr["target"] if with_chi else None     # chi of J_T_re, as a caller's
    got = rcf.evaluate(pr, pr["pulsevals"], functional=functional, D=D, lambda_b=lam, chi=chi)
    if with_chi:
        assert functional == 2
        assert _worst(got, want, ("G", "rhoT", "tau_grads", "J_b")) <= BOUND
    else:
        assert _worst(got, want, ("J", "tau", "G", "rhoT", "tau_grads", "J_b")) <= BOUND
        assert abs(got["J_T"] - want_T["J"]) <= BOUND
    assert np.abs(got["G_T"] - want_T["G"]).max() <= BOUND
    assert np.abs(got["G_T"] + lam * got["G_b"] - got["G"]).max() <= BOUND
    assert abs(np.sum(got["Jb_k"]) - got["J_b"]) <= BOUND


_cache = {}


def _ld_case(d):
    if d not in _cache:
        pr = _problem(d, 2, 2, K=2 if d == 4 else 1, N_T=3)
        oh.order_one_states(pr, 5100 + d)
        D = rcf.hermitian_D(88 + d, d)
        _cache[d] = (pr, D)
    return _cache[d]


@pytest.mark.parametrize("d", [4, 17])
def test_double_against_long_double(d):
    """the long-double side also runs on a finer sub-step rule (theta = 0.5 against 1)"""
    pr, D = _ld_case(d)
    got = rcf.evaluate(pr, pr["pulsevals"], functional=1, D=D, lambda_b=0.5)
    want = rcf.evaluate(pr, pr["pulsevals"], functional=1, D=D, lambda_b=0.5, dtype=np.clongdouble, theta=0.5)
    assert want["tau_grads"].dtype == np.clongdouble and np.finfo(np.longdouble).eps < 2e-19
    assert _worst(got, want, ("J", "J_T", "J_b", "tau", "G", "G_T", "G_b", "rhoT", "tau_grads")) <= BOUND


def test_a_nonlinear_caller_cost_against_central_differences():
    """g_b = -tr(rho^dagger rho) (loss of purity), xi = rho: dg_b = -2 Re <<rho | d rho>>.  The difference quotient of the
    reference's own J at h = 1e-5 has a truncation error of h^2 |J'''| / 6 ~ 1e-10 and a rounding error of eps / h ~ 1e-11."""
    pr, _ = _ld_case(4)
    cost = dict(g_b=lambda rho, k, m: -np.sum(np.abs(rho) ** 2), xi=lambda rho, k, m: rho)
    x, lam, h = pr["pulsevals"], 0.6, 1e-5
    got = rcf.evaluate(pr, x, functional=0, lambda_b=lam, **cost)
    fd = np.empty_like(x)
    for i in range(len(x)):
        e = np.zeros_like(x)
        e[i] = h
        fd[i] = (rcf.evaluate(pr, x + e, functional=0, lambda_b=lam, **cost)["J"] - rcf.evaluate(pr, x - e, functional=0, lambda_b=lam, **cost)["J"]) / (2 * h)
    print(dict(dG=float(np.abs(got["G"] - fd).max()), G=float(np.abs(got["G"]).max()), Gb=float(np.abs(got["G_b"]).max())))
    assert np.abs(got["G_b"]).max() >= 1e-3
    assert np.abs(got["G"] - fd).max() <= 2e-9


# ---- the comparison must notice a wrong side ------------------------------------------------------------------------------
def _mutation_case():
    """d = 5, K = 2, a complex Hermitian D per trajectory, a non-uniform grid whose middle interval the reference cuts"""
    if "mut" not in _cache:
        from grape_jl_amd import synth
        pr = synth.make_open_problem(5, 2, 3, 2, 2, seed=4242)
        pr["tlist"] = np.array([0.0, 0.7, 2.9, 3.4])
        pr["weights"] = np.array([0.8, 1.3])
        oh.order_one_states(pr, 4242)
        D = rcf.hermitian_D(4242, 5, 2)
        assert np.abs(D - np.swapaxes(D, -1, -2)).max() > 0.1 and np.abs(D[0] - D[1]).max() > 0.1
        good = rcf.evaluate(pr, pr["pulsevals"], functional=1, D=D, lambda_b=1.0)
        lam = rcf.lambda_from(good)
        good = rcf.evaluate(pr, pr["pulsevals"], functional=1, D=D, lambda_b=lam)
        rcf.assert_order_one(good, lam)
        assert good["substeps"][:, 1].min() >= 2
        _cache["mut"] = (pr, D, lam, good)
    return _cache["mut"]


def test_the_comparison_accepts_the_reference_itself():
    pr, D, lam, good = _mutation_case()
    rcf.assert_runcost_agrees(good, good)


@pytest.mark.parametrize("mutation", rcf.MUTATIONS)
def test_the_comparison_refuses_a_wrong_reference(mutation):
    pr, D, lam, good = _mutation_case()
    wrong = rcf.evaluate(pr, pr["pulsevals"], functional=1, D=D, lambda_b=lam, mutate=mutation)
    with pytest.raises(AssertionError):
        rcf.assert_runcost_agrees(good, wrong, mutation)
