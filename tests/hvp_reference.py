"""Reference for exact Hessian-vector products of J (tests/test_hvp_reference.py proves it, tests/test_gpu_hvp.py uses it).

numpy / scipy only, nothing of the product path, and a different formula from the kernels': full propagators from
``scipy.linalg.expm``, first derivatives ``DU[X]`` from ``expm_frechet``, the mixed second derivative ``D^2 U[D_l, B]`` as the
top-right block of ``expm`` of the 4 x 4 block matrix
    [[A, D_l, B, 0], [0, A, 0, B], [0, 0, A, D_l], [0, 0, 0, A]],
and the result assembled with explicit Psi' and chi':
    A = -i H_kn dt_n,   D_l = -i s_ln dt_n H_l,   B = sum_l v_nl D_l
    Psi_n  = U_n Psi_{n-1},                 Psi'_n  = U_n Psi'_{n-1} + DU_n[B] Psi_{n-1}
    chi_{n-1} = U_n^+ chi_n,                chi'_{n-1} = U_n^+ chi'_n + DU_n[B]^+ chi_n
    G_nl      = -2 Re sum_k <chi_n | DU_n[D_l] Psi_{n-1}>
    (H v)_nl  = -2 Re sum_k [ <chi'_n | DU_n[D_l] Psi_{n-1}> + <chi_n | D^2U_n[D_l, B] Psi_{n-1}> + <chi_n | DU_n[D_l] Psi'_{n-1}> ]
with chi(T) = c_k tgt_k and chi'(T) = c'_k tgt_k of the three functionals (include/grape_hip.h).

``wrong=`` switches ONE deliberate mistake on (the refusal tests of the shared comparison).
"""
import numpy as np
from scipy.linalg import expm, expm_frechet

WRONG = ("drop_d2u", "zero_chi_prime", "drop_psi_prime", "shape_shift", "ignore_last_weight")


def tol_hv(Hv):
    """the project's gradient tolerance applied to H v (tests/open_helpers.py: tol_G)"""
    return 1e-10 * max(float(np.abs(Hv).max()), 1e-3)


def assert_hvp_agrees(got, want, label=""):
    """THE comparison of the H v tests: ||got - want||_inf <= 1e-10 max(||want||_inf, 1e-3)"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got))
    dev, tol = float(np.abs(got - want).max()), tol_hv(want)
    print(label, dict(dHv=dev, tol=tol, Hv_max=float(np.abs(want).max())))
    assert dev <= tol, (label, dev, tol)
    return dev


def _coefficients(functional, tau, dtau, w, K):
    """c_k, c'_k of chi_k(T) = c_k tgt_k"""
    if functional == 0:
        return w * np.sum(w * tau) / K ** 2, w * np.sum(w * dtau) / K ** 2
    if functional == 1:
        return w * tau / K, w * dtau / K
    return w / (2.0 * K) + 0j * tau, 0j * tau


def _d2u(A, D, B):
    N = A.shape[0]
    Z = np.zeros_like(A)
    M = np.block([[A, D, B, Z], [Z, A, Z, B], [Z, Z, A, D], [Z, Z, Z, A]])
    return expm(M)[:N, 3 * N:]


def evaluate(pr, x, V, functional=0, wrong=None):
    """J, G [L*N_T], tau [K] and Hv [nv, L*N_T] (or [L*N_T] for a 1-D V) at the pulses x (control-major)."""
    assert wrong is None or wrong in WRONG
    H0, Hc = np.asarray(pr["H0"], dtype=complex), np.asarray(pr["Hc"], dtype=complex)
    psi0, target = np.asarray(pr["psi0"], dtype=complex), np.asarray(pr["target"], dtype=complex)
    tlist = np.asarray(pr["tlist"], dtype=float)
    K, N = psi0.shape
    L = Hc.shape[-3]
    N_T = len(tlist) - 1
    w = np.ones(K) if pr.get("weights") is None else np.array(pr["weights"], dtype=float)
    if wrong == "ignore_last_weight":
        w[-1] = 1.0
    S = np.ones((L, N_T)) if pr.get("shape") is None else np.asarray(pr["shape"], dtype=float).reshape(L, N_T)
    eps = np.asarray(x, dtype=float).reshape(L, N_T)
    Vs = np.asarray(V, dtype=float)
    one = Vs.ndim == 1
    Vs = Vs.reshape(-1, L, N_T)
    hck = (lambda k: Hc[k]) if Hc.ndim == 4 else (lambda k: Hc)
    dts = np.diff(tlist)

    # per (k, n): U, DU[D_l]; per direction additionally DU[B], D^2U[D_l, B]
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
    tau = np.einsum("ki,ki->k", target.conj(), psi[:, -1])
    f = np.sum(w * tau)
    J = [1.0 - abs(f) ** 2 / K ** 2, 1.0 - np.sum(w * np.abs(tau) ** 2) / K, 1.0 - np.real(f) / K][functional]

    G = np.zeros((L, N_T))
    Hv = np.zeros((len(Vs), L, N_T))
    for j, v in enumerate(Vs):
        Sb = np.roll(S, -1, axis=0) if wrong == "shape_shift" else S     # the shape of control l + 1 applied to l
        dUB = np.empty((K, N_T, N, N), complex)
        Bgen = np.empty((K, N_T, N, N), complex)
        for k in range(K):
            for n in range(N_T):
                Bgen[k, n] = sum(v[l, n] * (-1j * dts[n] * Sb[l, n] * hck(k)[l]) for l in range(L))
                dUB[k, n] = expm_frechet(Agen[k, n], Bgen[k, n], compute_expm=False)
        dpsi = np.zeros((K, N_T + 1, N), complex)
        for k in range(K):
            for n in range(N_T):
                dpsi[k, n + 1] = U[k, n] @ dpsi[k, n] + dUB[k, n] @ psi[k, n]
        dtau = np.einsum("ki,ki->k", target.conj(), dpsi[:, -1])
        c, dc = _coefficients(functional, tau, dtau, w, K)
        if wrong == "zero_chi_prime":
            dc = 0 * dc
        for k in range(K):
            chi, dchi = c[k] * target[k], dc[k] * target[k]
            for n in range(N_T - 1, -1, -1):
                for l in range(L):
                    if j == 0:
                        G[l, n] += -2.0 * np.real(np.vdot(chi, dU[k, n, l] @ psi[k, n]))
                    t = np.vdot(dchi, dU[k, n, l] @ psi[k, n])
                    if wrong != "drop_d2u":
                        t += np.vdot(chi, _d2u(Agen[k, n], Dl[k, n, l], Bgen[k, n]) @ psi[k, n])
                    if wrong != "drop_psi_prime":
                        t += np.vdot(chi, dU[k, n, l] @ dpsi[k, n])
                    Hv[j, l, n] += -2.0 * np.real(t)
                chi, dchi = U[k, n].conj().T @ chi, U[k, n].conj().T @ dchi + dUB[k, n].conj().T @ chi
    Hv = Hv.reshape(len(Vs), L * N_T)
    return dict(J=float(J), G=G.reshape(-1), tau=tau, Hv=Hv[0] if one else Hv, psiT=psi[:, -1])


def order_one_targets(pr, factor=0.8):
    """targets with O(1) signals, in place: the normalised Psi_k(T) of the pulse factor * x (as the open-system tests do)"""
    other = dict(pr)
    other["target"] = np.asarray(pr["psi0"])
    psiT = evaluate(other, factor * np.asarray(pr["pulsevals"]), np.zeros_like(pr["pulsevals"]))["psiT"]
    pr["target"] = psiT / np.linalg.norm(psiT, axis=1, keepdims=True)
    return pr


def assert_order_one(want):
    """the conditions on the REFERENCE alone under which the bound of assert_hvp_agrees is relative, never its floor"""
    fig = dict(tau_min=float(np.abs(want["tau"]).min()), G_max=float(np.abs(want["G"]).max()), Hv_max=float(np.abs(want["Hv"]).max()))
    print(fig)
    assert fig["tau_min"] >= 0.1
    assert fig["G_max"] >= 1e-3
    assert fig["Hv_max"] >= 1e-3
    return fig


def directions(seed, nv, n):
    """nv deterministic O(1) directions of length n"""
    from grape_jl_amd import synth
    return 2.0 * synth.uniform01(synth.subseed(seed, 9100), nv * n).reshape(nv, n) - 1.0
