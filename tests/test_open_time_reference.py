"""Proof of tests/open_time_reference.py, the reference of grape_open_time_gradient -- no GPU needed.

The forward-sensitivity reference is compared with 4th-order central differences of open_reference.evaluate()["J"] over every
dt_n, with scipy.linalg.expm of the d^2 x d^2 generator, with itself in long double and at another sub-step threshold, and with
a numpy transcription of the kernel's adjoint form (chi stepped back, <<L^dagger chi_{n+1} | rho_{n+1}>>).  The shared
comparison assert_time_gradient_agrees must refuse six deliberately wrong versions of that form.

Measured with these inputs (worst over the cases): central differences 7.1e-12 absolute at ||dJ/d dt||_inf = 0.006 ... 0.06
(bound 1e-10, 14 times that); expm 5.6e-16 (bound 1e-13); long double and theta 3.5e-17 (bound 1e-14); adjoint form 4.2e-17
(bound 1e-14).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402
import open_reference as orf  # noqa: E402
import open_time_reference as otr  # noqa: E402
from open_time_reference import RE, SM, SS  # noqa: E402


def _small(d, J, functional, **kw):
    spec = dict(d=d, J=J, L=2, K=2, functional=functional, weights=True, shape=True, nonuniform=True)
    spec.update(kw)
    return otr.build_case(spec)


# ---- central differences of J ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", [SM, SS, RE], ids=["sm", "ss", "re"])
@pytest.mark.parametrize("J", [0, 2, 3])
@pytest.mark.parametrize("d", [3, 4, 5])
def test_against_central_differences_of_J(d, J, functional):
    pr = _small(d, J, functional)
    x, h = pr["pulsevals"], 1e-4
    got = otr.time_gradient(pr, x, functional)
    dts = np.diff(pr["tlist"])
    fd = np.empty(len(dts))
    for n in range(len(dts)):
        def Jat(step):
            q = dts.copy()
            q[n] += step
            return orf.evaluate(pr, x, functional=functional, tlist=np.concatenate([[0.0], np.cumsum(q)]))["J"]
        fd[n] = (-Jat(2 * h) + 8 * Jat(h) - 8 * Jat(-h) + Jat(-2 * h)) / (12 * h)
    dev = np.abs(got - fd).max()
    print(dict(d=d, J=J, functional=functional, dev=dev, size=np.abs(fd).max()))
    assert np.abs(fd).max() >= 1e-3
    assert dev <= 1e-10


# ---- scipy.linalg.expm of the d^2 x d^2 generator ------------------------------------------------------------------------------
@pytest.mark.parametrize("d,J", [(2, 0), (2, 3), (4, 3), (4, 8), (5, 0), (5, 8)])
def test_against_expm_of_the_super_generator(d, J):
    """term[k][n] = vec(chi_k)^dagger Phi_after L_n Phi_upto vec(rho_k(0)), operators per trajectory, non-Hermitian drift and states"""
    import scipy.linalg
    pr = _small(d, J, SS, cops_per_traj=J > 0, hc_per_traj=True, hermitian=False, non_hermitian_states=0.3)
    x = pr["pulsevals"]
    parts = otr.time_gradient(pr, x, SS, want_parts=True)
    K, L, N_T = 2, 2, 3
    dts = np.diff(pr["tlist"])
    e = (pr["shape"] * x.reshape(L, N_T))
    terms = np.empty((K, N_T), complex)
    tau = np.empty(K, complex)
    for k in range(K):
        cops = list(pr["cops"][k]) if J else []
        gens = [-1j * oh.super_generator(pr["H0"][k] + sum(e[l, n] * pr["Hc"][k, l] for l in range(L)), cops) for n in range(N_T)]
        phis = [scipy.linalg.expm(gens[n] * dts[n]) for n in range(N_T)]
        v = [oh.vec(pr["rho0"][k])]
        for n in range(N_T):
            v.append(phis[n] @ v[-1])
        tau[k] = np.vdot(oh.vec(pr["target"][k]), v[-1])
        for n in range(N_T):
            u = gens[n] @ v[n + 1]
            for q in range(n + 1, N_T):
                u = phis[q] @ u
            terms[k, n] = np.vdot(oh.vec(pr["target"][k]), u)
    _, c = orf.functional_values(tau, pr["weights"], SS)
    want = -2 * np.sum(np.conj(c)[:, None] * terms, axis=0).real
    dev = np.abs(parts["dJdt"] - want).max()
    print(dict(d=d, J=J, dev=dev, size=np.abs(want).max()))
    assert np.abs(parts["tau"] - tau).max() <= 1e-13
    assert dev <= 1e-13


# ---- precision ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,J", [(4, 2), (17, 8)])
def test_double_against_long_double_and_another_theta(d, J):
    pr = _small(d, J, SM, factor=-0.8 if J == 8 else 0.8)
    x = pr["pulsevals"]
    a = otr.time_gradient(pr, x, SM)
    b = otr.time_gradient(pr, x, SM, dtype=np.clongdouble)
    c = otr.time_gradient(pr, x, SM, theta=0.5)
    dev = max(float(np.abs(a - b).max()), float(np.abs(a - c).max()))
    print(dict(d=d, long_double=float(np.abs(a - b).max()), theta=float(np.abs(a - c).max()), size=np.abs(a).max()))
    assert b.dtype == np.longdouble
    assert dev <= 1e-14


# ---- the kernel's form, transcribed -----------------------------------------------------------------------------------------
def adjoint_form(pr, pulsevals, functional, mutation=None, theta=1.0):
    """chi stepped back from chi_k(T) = c_k sigma_k with L^dagger; dJdt[n] = -2 Re sum_k <<L_kn^dagger chi_k(t_{n+1}) | rho_k(t_{n+1})>>.
    ``mutation`` makes it subtly wrong (test_the_comparison_refuses_wrong_references)."""
    dtype, tol = np.complex128, 1e-18
    H0, Hc_all = np.asarray(pr["H0"], dtype), np.asarray(pr["Hc"], dtype)
    K, d = H0.shape[0], H0.shape[1]
    L = Hc_all.shape[-3]
    cops_all = np.asarray(pr["cops"], dtype)
    tl = np.asarray(pr["tlist"], float)
    N_T = len(tl) - 1
    eps = np.asarray(pulsevals, float).reshape(L, N_T)
    s = np.ones((L, N_T)) if pr.get("shape") is None else np.asarray(pr["shape"], float)
    w = np.ones(K) if pr.get("weights") is None else np.array(pr["weights"], float)
    if mutation == "last weight ignored":
        w[-1] = 1.0

    def lind_of(M, cops, adjoint):
        copsd = orf._dag(cops)
        if adjoint:
            M, cops, copsd = orf._dag(M), copsd, cops

        def apply(X):
            out = M @ X + X @ orf._dag(M)
            for j in range(len(cops)):
                out = out + cops[j] @ X @ copsd[j]
            return out
        return apply

    store, gens = [], []
    for k in range(K):
        Hc, cops = orf._per_k(Hc_all, k, 3), orf._per_k(cops_all, k, 3)
        AdA = sum((orf._dag(A) @ A for A in cops), np.zeros((d, d), dtype))
        Ms = [-1j * (H0[k] + sum(s[l, n] * eps[l, n] * Hc[l] for l in range(L))) - AdA / 2 for n in range(N_T)]
        rhos = [np.asarray(pr["rho0"], dtype)[k][None]]
        for n in range(N_T):
            dt = tl[n + 1] - tl[n]
            m = orf.substeps(Ms[n], cops, dt, theta)
            Y = rhos[-1]
            for _ in range(m):
                Y = orf._series(lind_of(Ms[n], cops, False), Y, dt / m, tol, None)
            rhos.append(Y)
        store.append(rhos)
        gens.append((Ms, cops, Hc, AdA))
    target = np.asarray(pr["target"], dtype)
    tau = np.array([np.sum(np.conj(target[k]) * store[k][-1][0]) for k in range(K)])
    _, c = orf.functional_values(tau, w, functional)
    terms = np.empty((K, N_T), complex)
    for k in range(K):
        Ms, cops, Hc, AdA = gens[k]
        chi = (c[k] * target[k])[None]
        for n in range(N_T - 1, -1, -1):
            nn = min(n + 1, N_T - 1) if mutation == "generator of interval n + 1" else n
            Mo, co = Ms[nn], cops
            if mutation == "dissipator left out":
                Mo, co = Ms[n] + AdA / 2, cops[:0]
            if mutation == "shape dropped":
                Mo = -1j * (H0[k] + sum(eps[l, n] * Hc[l] for l in range(L))) - AdA / 2
            rho = store[k][n][0] if mutation == "rho(t_n)" else store[k][n + 1][0]
            terms[k, n] = np.sum(np.conj(lind_of(Mo, co, True)(chi)[0]) * rho)
            dt = tl[n + 1] - tl[n]
            m = orf.substeps(Ms[n], cops, dt, theta)
            for _ in range(m):
                chi = orf._series(lind_of(Ms[n], cops, True), chi, dt / m, tol, None)
    out = -2 * np.sum(terms, axis=0).real
    return out[::-1].copy() if mutation == "interval order reversed" else out


@pytest.mark.parametrize("functional", [SM, SS, RE], ids=["sm", "ss", "re"])
@pytest.mark.parametrize("d,J", [(4, 2), (5, 3), (17, 8)])
def test_adjoint_form_agrees_with_the_forward_form(d, J, functional):
    pr = _small(d, J, functional, factor=-0.8 if J == 8 else 0.8)
    a = otr.time_gradient(pr, pr["pulsevals"], functional)
    b = adjoint_form(pr, pr["pulsevals"], functional)
    print(dict(d=d, J=J, functional=functional, dev=np.abs(a - b).max(), size=np.abs(a).max()))
    assert np.abs(a - b).max() <= 1e-14


@pytest.mark.parametrize("functional", [SM, SS, RE], ids=["sm", "ss", "re"])
def test_callers_chi_reproduces_the_builtin_result(functional):
    pr = _small(5, 3, functional)
    parts = otr.time_gradient(pr, pr["pulsevals"], functional, want_parts=True)
    _, c = orf.functional_values(parts["tau"], pr["weights"], functional)
    chi = np.asarray(c, complex)[:, None, None] * pr["target"]
    got = otr.time_gradient(pr, pr["pulsevals"], functional, boundary=chi)
    assert np.abs(got - parts["dJdt"]).max() <= 1e-15


MUTATIONS = ["dissipator left out", "generator of interval n + 1", "rho(t_n)", "shape dropped", "last weight ignored",
             "interval order reversed"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_comparison_refuses_wrong_references(mutation):
    pr = _small(5, 3, SM, K=3)      # (weights 0.5, 1.0, 1.5: the last one is not 1)
    parts = otr.time_gradient(pr, pr["pulsevals"], SM, want_parts=True)
    otr.assert_time_gradient_agrees(adjoint_form(pr, pr["pulsevals"], SM), parts["dJdt"], parts["tau"], "unmutated")
    wrong = adjoint_form(pr, pr["pulsevals"], SM, mutation=mutation)
    with pytest.raises(AssertionError):
        otr.assert_time_gradient_agrees(wrong, parts["dJdt"], parts["tau"], mutation)
    # ... and by a wide margin, not by an accident of rounding
    assert np.abs(wrong - parts["dJdt"]).max() >= 1e3 * otr.tol_time(parts["dJdt"])


def test_the_comparison_insists_on_order_one_signals():
    with pytest.raises(AssertionError):
        otr.assert_time_gradient_agrees(np.full(3, 1e-5), np.full(3, 1e-5), np.ones(2))
    with pytest.raises(AssertionError):
        otr.assert_time_gradient_agrees(np.full(3, 0.1), np.full(3, 0.1), np.array([1.0, 0.05]))
    otr.assert_time_gradient_agrees(np.full(3, 0.1), np.full(3, 0.1), np.ones(2))
