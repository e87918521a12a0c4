"""Reference for Hessian-vector products of a CALLER'S functional (tests/test_hvp_split_reference.py proves it,
tests/test_gpu_hvp_split.py uses it).

Built from the blocks of tests/hvp_reference.py -- ``expm``, ``expm_frechet`` and the 4 x 4 block exponential ``_d2u`` -- with
the boundary of the backward recursion left to a callback, as grape_hvp_forward + grape_hvp_backward_chi leave it to the caller:

    boundary(psiT [K, N], dpsiT_j [K, N]) -> (J, chi [K, N], dchi_j [K, N])

with chi_k = -dJ/d<Psi_k(T)| (not normalised) and dchi_j its derivative along direction j.  Works with ``pr["target"] is None``
(then ``tau`` and ``dtau`` are None).

``wrong=`` switches ONE deliberate mistake on (the refusal tests of the shared comparison).
"""
import numpy as np
from scipy.linalg import expm, expm_frechet

import hvp_reference as hr

WRONG = ("zero_dchi", "dchi_from_psi", "drop_psi_prime")


def evaluate_chi(pr, x, V, boundary, wrong=None):
    """J, G [L*N_T], Hv [nv, L*N_T] (or [L*N_T] for a 1-D V), psiT [K, N], dpsiT [nv, K, N], tau [K] and dtau [nv, K] (None
    without targets) at the pulses x (control-major)."""
    assert wrong is None or wrong in WRONG
    H0, Hc = np.asarray(pr["H0"], dtype=complex), np.asarray(pr["Hc"], dtype=complex)
    psi0 = np.asarray(pr["psi0"], dtype=complex)
    target = None if pr.get("target") is None else np.asarray(pr["target"], dtype=complex)
    tlist = np.asarray(pr["tlist"], dtype=float)
    K, N = psi0.shape
    L = Hc.shape[-3]
    N_T = len(tlist) - 1
    S = np.ones((L, N_T)) if pr.get("shape") is None else np.asarray(pr["shape"], dtype=float).reshape(L, N_T)
    eps = np.asarray(x, dtype=float).reshape(L, N_T)
    Vs = np.asarray(V, dtype=float)
    one = Vs.ndim == 1
    Vs = Vs.reshape(-1, L, N_T)
    hck = (lambda k: Hc[k]) if Hc.ndim == 4 else (lambda k: Hc)
    dts = np.diff(tlist)

    U = np.empty((K, N_T, N, N), complex)
    dU = np.empty((K, N_T, L, N, N), complex)
    Dl = np.empty((K, N_T, L, N, N), complex)
    Agen = np.empty((K, N_T, N, N), complex)
    for k in range(K):
        for n in range(N_T):
            H = H0[k] + sum(eps[l, n] * S[l, n] * hck(k)[l] for l in range(L))
            Agen[k, n] = -1j * dts[n] * H
            U[k, n] = expm(Agen[k, n])
            for l in range(L):
                Dl[k, n, l] = -1j * dts[n] * S[l, n] * hck(k)[l]
                dU[k, n, l] = expm_frechet(Agen[k, n], Dl[k, n, l], compute_expm=False)
    psi = np.empty((K, N_T + 1, N), complex)
    psi[:, 0] = psi0
    for k in range(K):
        for n in range(N_T):
            psi[k, n + 1] = U[k, n] @ psi[k, n]
    psiT = psi[:, -1].copy()

    J = None
    G = np.zeros((L, N_T))
    Hv = np.zeros((len(Vs), L, N_T))
    dpsiT = np.zeros((len(Vs), K, N), complex)
    for j, v in enumerate(Vs):
        dUB = np.empty((K, N_T, N, N), complex)
        Bgen = np.empty((K, N_T, N, N), complex)
        for k in range(K):
            for n in range(N_T):
                Bgen[k, n] = sum(v[l, n] * Dl[k, n, l] for l in range(L))
                dUB[k, n] = expm_frechet(Agen[k, n], Bgen[k, n], compute_expm=False)
        dpsi = np.zeros((K, N_T + 1, N), complex)
        for k in range(K):
            for n in range(N_T):
                dpsi[k, n + 1] = U[k, n] @ dpsi[k, n] + dUB[k, n] @ psi[k, n]
        dpsiT[j] = dpsi[:, -1]
        Jj, chiT, dchiT = boundary(psiT.copy(), (psiT if wrong == "dchi_from_psi" else dpsiT[j]).copy())
        chiT, dchiT = np.asarray(chiT, dtype=complex), np.asarray(dchiT, dtype=complex)
        assert chiT.shape == (K, N) and dchiT.shape == (K, N)
        if wrong == "zero_dchi":
            dchiT = 0 * dchiT
        J = float(Jj) if J is None else J
        for k in range(K):
            chi, dchi = chiT[k], dchiT[k]
            for n in range(N_T - 1, -1, -1):
                for l in range(L):
                    if j == 0:
                        G[l, n] += -2.0 * np.real(np.vdot(chi, dU[k, n, l] @ psi[k, n]))
                    t = np.vdot(dchi, dU[k, n, l] @ psi[k, n])
                    t += np.vdot(chi, hr._d2u(Agen[k, n], Dl[k, n, l], Bgen[k, n]) @ psi[k, n])
                    if wrong != "drop_psi_prime":
                        t += np.vdot(chi, dU[k, n, l] @ dpsi[k, n])
                    Hv[j, l, n] += -2.0 * np.real(t)
                chi, dchi = U[k, n].conj().T @ chi, U[k, n].conj().T @ dchi + dUB[k, n].conj().T @ chi
    Hv = Hv.reshape(len(Vs), L * N_T)
    tau = dtau = None
    if target is not None:
        tau = np.einsum("ki,ki->k", target.conj(), psiT)
        dtau = np.einsum("ki,jki->jk", target.conj(), dpsiT)
    return dict(J=J, G=G.reshape(-1), Hv=Hv[0] if one else Hv, psiT=psiT, dpsiT=dpsiT, tau=tau, dtau=dtau)


def builtin_boundary(pr, functional):
    """the three built-in functionals (include/grape_hip.h) written as a caller's boundary"""
    target = np.asarray(pr["target"], dtype=complex)
    K = target.shape[0]
    w = np.ones(K) if pr.get("weights") is None else np.array(pr["weights"], dtype=float)

    def boundary(psiT, dpsiT):
        tau = np.einsum("ki,ki->k", target.conj(), psiT)
        dtau = np.einsum("ki,ki->k", target.conj(), dpsiT)
        f = np.sum(w * tau)
        J = [1.0 - abs(f) ** 2 / K ** 2, 1.0 - np.sum(w * np.abs(tau) ** 2) / K, 1.0 - np.real(f) / K][functional]
        c, dc = hr._coefficients(functional, tau, dtau, w, K)
        return J, c[:, None] * target, dc[:, None] * target
    return boundary


def observables(seed, K, N):
    """O_k of the expectation-value functional: one GUE matrix per trajectory"""
    from grape_jl_amd import synth
    return np.stack([synth.gue(synth.subseed(seed, 900 + k), N) for k in range(K)])


def expectation_boundary(O, weights=None):
    """J = sum_k w_k Re <Psi_k(T)| O_k |Psi_k(T)> / K,  chi_k = -w_k O_k Psi_k(T) / K,  chi'_k = -w_k O_k Psi'_k(T) / K"""
    K = O.shape[0]
    w = np.ones(K) if weights is None else np.array(weights, dtype=float)

    def boundary(psiT, dpsiT):
        Opsi = np.einsum("kij,kj->ki", O, psiT)
        J = float(np.sum(w * np.real(np.einsum("ki,ki->k", psiT.conj(), Opsi))) / K)
        return J, -w[:, None] * Opsi / K, -w[:, None] * np.einsum("kij,kj->ki", O, dpsiT) / K
    return boundary


def assert_signals(want):
    """on the REFERENCE alone: ||G||_inf, ||Hv||_inf >= 1e-3, so that the bound of assert_hvp_agrees is relative, never its floor"""
    fig = dict(G_max=float(np.abs(want["G"]).max()), Hv_max=float(np.abs(want["Hv"]).max()))
    print(fig)
    assert fig["G_max"] >= 1e-3 and fig["Hv_max"] >= 1e-3
    return fig
