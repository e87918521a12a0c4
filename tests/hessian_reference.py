"""Reference for the exact Hessian of J as a matrix (tests/test_hessian_reference.py proves it against tests/hvp_reference.py,
tests/test_gpu_hessian.py uses it).

numpy / scipy only, nothing of the product path: full propagators from ``scipy.linalg.expm``, first derivatives ``DU[X]`` from
``expm_frechet``, the second derivative ``D^2 U[D_l, D_l']`` as the top-right block of the 4 x 4 block exponential of
``hvp_reference._d2u``.  Per trajectory, with 0-based intervals and U_n: t_n -> t_{n+1},
    A_n = -i dt_n H_kn,   D_nl = -i dt_n s_ln H_l
    theta_k(T) = tgt_k,   theta_k(t_n) = U_n^+ theta_k(t_{n+1})          the bare target chain
    a_(n,l)    = DU_n[D_nl] Psi_k(t_n)                                   lives at t_{n+1}
    beta_(n,l) = DU_n[D_nl]^+ theta_k(t_{n+1})                           lives at t_n
    T_k,p      = d tau_k / d eps_p = <beta_p | Psi_k(t_n)>               p = (n, l)
    S_k,pq     = <beta_(n,l) | U_{n-1} ... U_{m+1} a_(m,l')>             m < n
               = <theta_k(t_{n+1}) | D^2U_n[D_nl, D_nl'] Psi_k(t_n)>     m = n;     symmetric in p <-> q
    G_p  = -2 Re sum_k conj(c_k) T_k,p                                   chi_k(T) = c_k tgt_k (include/grape_hip.h)
    H_pq = -2 Re sum_k [ conj(c_k) S_k,pq + conj(d_q c_k) T_k,p ]
           sm: d_q c_k = w_k F_q / K_total^2, F_q = sum_j w_j T_j,q;   ss: d_q c_k = w_k T_k,q / K_total;   re: 0
The result is indexed like G: p = l * N_T + n.

The fan carries all live columns of a trajectory in one array, one matrix product per grid point.  It replaced a loop over
birth interval, grid point and both controls; on the five shapes of tests/test_hessian_reference.py the two agreed to
2.6e-16 ||H||_inf (bit for bit at N4-L4-NT5-K2-re), for every ``wrong=`` switch as well (4.8e-16 at most).

``wrong=`` switches ONE deliberate mistake on (the refusal tests of the shared comparison).
"""
import numpy as np
from scipy.linalg import expm, expm_frechet

from hvp_reference import _d2u

WRONG = ("drop_diagonal_blocks", "drop_boundary", "fan_one_interval_too_many", "k_for_k_total", "ignore_last_weight")


def tol_hessian(H):
    """the project's gradient tolerance applied to the entries of H (tests/hvp_reference.py: tol_hv)"""
    return 1e-10 * max(float(np.abs(H).max()), 1e-3)


def assert_hessian_agrees(got, want, label=""):
    """THE comparison of the Hessian tests: ||got - want||_inf <= 1e-10 max(||want||_inf, 1e-3), over all entries"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got))
    dev, tol = float(np.abs(got - want).max()), tol_hessian(want)
    print(label, dict(dH=dev, tol=tol, H_max=float(np.abs(want).max())))
    assert dev <= tol, (label, dev, tol)
    return dev


def evaluate(pr, x, functional=0, K_total=None, wrong=None):
    """J, G [L*N_T], tau [K] and H [L*N_T, L*N_T] at the pulses x (control-major).  ``K_total``: the trajectories of the
    whole problem (default: those of ``pr``).  The 4N x 4N exponentials of the diagonal blocks are taken for l' <= l alone and
    mirrored."""
    assert wrong is None or wrong in WRONG
    H0, Hc = np.asarray(pr["H0"], dtype=complex), np.asarray(pr["Hc"], dtype=complex)
    psi0, target = np.asarray(pr["psi0"], dtype=complex), np.asarray(pr["target"], dtype=complex)
    tlist = np.asarray(pr["tlist"], dtype=float)
    K, N = psi0.shape
    L = Hc.shape[-3]
    N_T = len(tlist) - 1
    Kt = float(K if K_total is None else K_total)
    if wrong == "k_for_k_total":
        Kt = float(K)
    w = np.ones(K) if pr.get("weights") is None else np.array(pr["weights"], dtype=float)
    if wrong == "ignore_last_weight":
        w[-1] = 1.0
    S = np.ones((L, N_T)) if pr.get("shape") is None else np.asarray(pr["shape"], dtype=float).reshape(L, N_T)
    eps = np.asarray(x, dtype=float).reshape(L, N_T)
    hck = (lambda k: Hc[k]) if Hc.ndim == 4 else (lambda k: Hc)
    dts = np.diff(tlist)
    P = L * N_T

    T = np.zeros((K, N_T, L), complex)               # T_k,(n,l)
    Sm = np.zeros((K, N_T, L, N_T, L), complex)       # S_k,(n,l)(m,l'), filled for (n, l) >= (m, l') and mirrored
    tau = np.zeros(K, complex)
    for k in range(K):
        U, A, D, dU = [], [], [], []
        for n in range(N_T):
            Hn = H0[k] + sum(eps[l, n] * S[l, n] * hck(k)[l] for l in range(L))
            A.append(-1j * dts[n] * Hn)
            U.append(expm(A[n]))
            D.append([-1j * dts[n] * S[l, n] * hck(k)[l] for l in range(L)])
            dU.append([expm_frechet(A[n], D[n][l], compute_expm=False) for l in range(L)])
        psi = [psi0[k]]
        for n in range(N_T):
            psi.append(U[n] @ psi[n])
        tau[k] = np.vdot(target[k], psi[-1])
        theta = [None] * (N_T + 1)
        theta[N_T] = target[k]
        for n in range(N_T - 1, -1, -1):
            theta[n] = U[n].conj().T @ theta[n + 1]
        a = [[dU[n][l] @ psi[n] for l in range(L)] for n in range(N_T)]
        beta = [[dU[n][l].conj().T @ theta[n + 1] for l in range(L)] for n in range(N_T)]
        for n in range(N_T):
            for l in range(L):
                T[k, n, l] = np.vdot(beta[n][l], psi[n])
                for l2 in range(l + 1):
                    if wrong != "drop_diagonal_blocks":
                        Sm[k, n, l, n, l2] = np.vdot(theta[n + 1], _d2u(A[n], D[n][l], D[n][l2]) @ psi[n])
                    Sm[k, n, l2, n, l] = Sm[k, n, l, n, l2]
        # the fan: the columns a_(m, .) are carried forwards and overlapped with beta_(n, .) at every later grid point.  All
        # live columns stand side by side (interval-major, q = m L + l'): one matrix product per grid point
        X = np.zeros((N, P), complex)
        rows_k, cols_k = Sm[k].reshape(N_T, L, P), Sm[k].reshape(P, N_T, L)     # (views) [n, l, q] and [q, n, l]
        for n in range(1, N_T):
            born = np.stack(a[n - 1], axis=1)         # at t_n
            if wrong == "fan_one_interval_too_many":
                born = U[n] @ born
            X[:, (n - 1) * L:n * L] = born
            ov = np.stack(beta[n], axis=1).conj().T @ X[:, :n * L]              # <beta_(n,l) | x_q>, q < n L
            rows_k[n, :, :n * L] = ov
            cols_k[:n * L, n, :] = ov.T
            if n + 1 < N_T:
                X[:, :n * L] = U[n] @ X[:, :n * L]

    f = np.sum(w * tau)
    J = [1.0 - abs(f) ** 2 / Kt ** 2, 1.0 - np.sum(w * np.abs(tau) ** 2) / Kt, 1.0 - np.real(f) / Kt][functional]
    c = [w * f / Kt ** 2, w * tau / Kt, w / (2.0 * Kt) + 0j * tau][functional]
    Tp, Sp = T.reshape(K, P), Sm.reshape(K, P, P)     # interval-major: (n, l) -> n L + l
    G = -2.0 * np.real(np.einsum("k,kp->p", c.conj(), Tp))
    Hm = np.real(np.einsum("k,kpq->pq", c.conj(), Sp))
    if wrong != "drop_boundary":
        if functional == 0:
            F = np.einsum("k,kq->q", w, Tp)
            dc = w[:, None] * F[None, :] / Kt ** 2      # [k, q]
        elif functional == 1:
            dc = w[:, None] * Tp / Kt
        else:
            dc = np.zeros((K, P), complex)
        Hm = Hm + np.real(np.einsum("kq,kp->pq", dc.conj(), Tp))
    Hm = -2.0 * Hm
    # (n, l) -> p = l N_T + n
    perm = np.array([n * L + l for l in range(L) for n in range(N_T)])
    return dict(J=float(J), G=G[perm], tau=tau, H=Hm[np.ix_(perm, perm)])


def assert_order_one(want):
    """the conditions on the REFERENCE alone under which the bound of assert_hessian_agrees is relative, never its floor"""
    fig = dict(tau_min=float(np.abs(want["tau"]).min()), G_max=float(np.abs(want["G"]).max()), H_max=float(np.abs(want["H"]).max()))
    print(fig)
    assert fig["tau_min"] >= 0.1
    assert fig["G_max"] >= 1e-3
    assert fig["H_max"] >= 1e-3
    return fig
