"""A plain matrix-form reference of the open-system evaluation (grape_create_open), independent of the kernels' algorithm:
numpy ``@`` products, generic over numpy.complex128 and numpy.clongdouble (x87 extended, eps = 1.1e-19).

    L(X) = M X + X M^dagger + sum_j A_j X A_j^dagger,      M = -i (H_kn - (i/2) sum_j A_j^dagger A_j)

Forward: the FORWARD sensitivity, not the adjoint block recursion of the kernels.  On interval n the pair (rho, s_l) obeys
    d rho / dt = L rho,      d s_l / dt = L s_l + shape_ln (D_l rho + rho D_l^dagger),   s_l(t_n) = 0,   D_l = -i H_l
so that s_l(t_{n+1}) = d rho(t_{n+1}) / d eps_nl.  The pair is summed as the Taylor series of its (linear) generator, on
m = ceil((2 ||M||_2 + sum_j ||A_j||_2^2) dt / theta) equal sub-steps (theta <= 1: a rule of its own, not the kernels'), every
series until ||term||_F <= tol ||sum||_F for every member of the pair: tol = 1e-18 in double, 1e-24 in long double.
Backward: the boundary matrix B_k (the target sigma_k, or a caller's chi_k) is stepped back with L^dagger alone, and
    base[k][l][n] = <<B_k(t_{n+1}) | s_l>> = tr(B_k(t_{n+1})^dagger s_l).
chi_k(T) = c_k sigma_k with the c_k of include/grape_hip.h, so tau_grads[k][l][n] = conj(c_k) base[k][l][n] and
G[l][n] = -2 Re sum_k tau_grads[k][l][n].
"""
import numpy as np

MAX_TERMS = 200


def _real(dtype):
    return np.longdouble if np.dtype(dtype) == np.dtype(np.clongdouble) else np.float64


def _fro(X):
    """Frobenius norm of every matrix of a stack [..., d, d] (numpy.linalg has no long-double kernels)"""
    return np.sqrt(np.sum(X.real * X.real + X.imag * X.imag, axis=(-2, -1)))


def _dag(X):
    return np.conj(np.swapaxes(X, -1, -2))


def _norm2(X):
    return float(np.linalg.norm(np.asarray(X, dtype=np.complex128), 2))


def generator_bound(M, cops):
    """beta = 2 ||M||_2 + sum_j ||A_j||_2^2 >= ||L||"""
    return 2.0 * _norm2(M) + sum(_norm2(A) ** 2 for A in cops)


def substeps(M, cops, dt, theta):
    """the reference's own sub-step rule"""
    return max(1, int(np.ceil(generator_bound(M, cops) * abs(float(dt)) / theta)))


def _series(apply, Y, h, tol, max_terms):
    """sum_a u_a, u_0 = Y, u_{a+1} = h / (a+1) apply(u_a), for a stack Y [m, d, d] whose members stop together"""
    total, u = Y.copy(), Y
    for a in range(MAX_TERMS if max_terms is None else max_terms):
        u = apply(u) * (h / (a + 1))
        total = total + u
        if max_terms is None and np.all(_fro(u) <= tol * _fro(total)):
            return total
    if max_terms is None:
        raise ArithmeticError("open_reference: a series did not converge (non-finite input?)")
    return total


def _per_k(a, k, ndim_shared):
    a = np.asarray(a)
    return a[k] if a.ndim == ndim_shared + 1 else a


def propagate(pr, pulsevals, boundary=None, shape=None, tlist=None, dtype=np.complex128, theta=1.0, gradient=True,
              max_terms=None):
    """Forward sweep of every trajectory and, with ``gradient``, the overlaps base[k][l][n] with ``boundary`` [K, d, d]
    (default: the targets) stepped back.  Returns dict(rhoT [K,d,d], base [K,L,N_T] or None), in ``dtype``.
    ``max_terms`` cuts every series at that many terms instead of summing it to convergence (tests of the tests only)."""
    rdt = _real(dtype)
    tol = rdt(1e-24) if rdt is np.longdouble else rdt(1e-18)
    H0 = np.asarray(pr["H0"], dtype=dtype)
    K, d = H0.shape[0], H0.shape[1]
    Hc_all = np.asarray(pr["Hc"], dtype=dtype)
    L = Hc_all.shape[-3]
    cops_all = np.zeros((0, d, d), dtype=dtype) if pr.get("cops") is None or np.size(pr["cops"]) == 0 else np.asarray(pr["cops"], dtype=dtype)
    tl = np.asarray(pr["tlist"] if tlist is None else tlist, dtype=rdt)
    N_T = len(tl) - 1
    eps = np.asarray(pulsevals, dtype=rdt).reshape(L, N_T)
    shape = pr.get("shape") if shape is None else shape
    s = np.ones((L, N_T), dtype=rdt) if shape is None else np.asarray(shape, dtype=rdt).reshape(L, N_T)
    rho0 = np.asarray(pr["rho0"], dtype=dtype)
    if gradient and boundary is None:
        boundary = pr["target"]
    im = dtype(1j)
    rhoT = np.empty((K, d, d), dtype=dtype)
    base = np.zeros((K, L, N_T), dtype=dtype) if gradient else None
    for k in range(K):
        Hc, cops = _per_k(Hc_all, k, 3), _per_k(cops_all, k, 3)
        copsd = _dag(cops)
        AdA = sum((copsd[j] @ cops[j] for j in range(len(cops))), np.zeros((d, d), dtype=dtype))
        D = -im * Hc
        Dd = _dag(D)
        Ms, ms, sens = [], [], []
        rho = rho0[k]
        for n in range(N_T):
            H = H0[k] + sum((s[l, n] * eps[l, n]) * Hc[l] for l in range(L))
            M = -im * H - AdA / 2
            Md = _dag(M)
            dt = tl[n + 1] - tl[n]
            m = substeps(M, cops, dt, theta)
            Ms.append(M)
            ms.append(m)

            def lind(X, M=M, Md=Md):
                out = M @ X + X @ Md
                for j in range(len(cops)):
                    out = out + cops[j] @ X @ copsd[j]
                return out

            if gradient:
                def pair(Y, n=n, lind=lind):
                    out = lind(Y)
                    for l in range(L):
                        out[1 + l] = out[1 + l] + s[l, n] * (D[l] @ Y[0] + Y[0] @ Dd[l])
                    return out
                Y = np.concatenate([rho[None], np.zeros((L, d, d), dtype=dtype)])
                for _ in range(m):
                    Y = _series(pair, Y, dt / m, tol, max_terms)
                rho = Y[0]
                sens.append(Y[1:])
            else:
                Y = rho[None]
                for _ in range(m):
                    Y = _series(lind, Y, dt / m, tol, max_terms)
                rho = Y[0]
        rhoT[k] = rho
        if not gradient:
            continue
        B = np.asarray(boundary, dtype=dtype)[k][None]
        for n in range(N_T - 1, -1, -1):
            base[k, :, n] = np.sum(np.conj(B) * sens[n], axis=(-2, -1))        # <<B(t_{n+1}) | s_l>>
            M, Md = Ms[n], _dag(Ms[n])

            def lind_adj(Y, M=M, Md=Md):
                out = Md @ Y + Y @ M
                for j in range(len(cops)):
                    out = out + copsd[j] @ Y @ cops[j]
                return out

            dt = tl[n + 1] - tl[n]
            for _ in range(ms[n]):
                B = _series(lind_adj, B, dt / ms[n], tol, max_terms)
    return dict(rhoT=rhoT, base=base)


def functional_values(tau, weights, functional):
    """J and the coefficients c_k of chi_k(T) = c_k sigma_k (include/grape_hip.h: J_T_sm = 0, J_T_ss = 1, J_T_re = 2)"""
    Kt = K = len(tau)
    w = np.ones(K, dtype=tau.real.dtype) if weights is None else np.asarray(weights, dtype=tau.real.dtype)
    f = np.sum(w * tau)
    if functional == 0:
        return 1 - (f.real * f.real + f.imag * f.imag) / Kt ** 2, w * f / Kt ** 2
    if functional == 1:
        return 1 - np.sum(w * (tau.real * tau.real + tau.imag * tau.imag)) / Kt, w * tau / Kt
    if functional == 2:
        return 1 - f.real / Kt, (w / (2 * Kt)).astype(tau.dtype)
    raise ValueError(f"functional {functional}")


def from_parts(parts, pr, functional, weights=None):
    """dict(J, G [L*N_T], tau [K], rhoT [K,d,d], tau_grads [K,L,N_T]) of one built-in functional from ``propagate``'s output"""
    rhoT, base = parts["rhoT"], parts["base"]
    target = np.asarray(pr["target"], dtype=rhoT.dtype)
    tau = np.sum(np.conj(target) * rhoT, axis=(-2, -1))
    weights = pr.get("weights") if weights is None else weights
    J, c = functional_values(tau, weights, functional)
    tg = np.conj(c)[:, None, None] * base
    G = -2 * np.sum(tg, axis=0).real
    return dict(J=J, G=G.reshape(-1), tau=tau, rhoT=rhoT, tau_grads=tg)


def evaluate(pr, pulsevals, functional=0, weights=None, shape=None, tlist=None, dtype=np.complex128, theta=1.0, max_terms=None):
    """The reference of GrapeHipOpen.eval(..., want_psiT=True) + tau_grads() for the problem dicts of the open-system tests:
    H0 [K,d,d], Hc [L,d,d] or [K,L,d,d], cops None / [J,d,d] / [K,J,d,d], rho0, target [K,d,d], tlist, and optionally
    shape [L,N_T], weights [K] (arguments override the dict's).  pulsevals is control-major [l * N_T + n]."""
    parts = propagate(pr, pulsevals, shape=shape, tlist=tlist, dtype=dtype, theta=theta, max_terms=max_terms)
    return from_parts(parts, pr, functional, weights)


def evaluate_chi(pr, pulsevals, chi, shape=None, tlist=None, dtype=np.complex128, theta=1.0):
    """The reference of forward + final_states + backward_chi(chi): dict(G, rhoT, tau_grads)"""
    parts = propagate(pr, pulsevals, boundary=chi, shape=shape, tlist=tlist, dtype=dtype, theta=theta)
    return dict(G=(-2 * np.sum(parts["base"], axis=0).real).reshape(-1), rhoT=parts["rhoT"], tau_grads=parts["base"])
