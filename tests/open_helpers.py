"""Shared pieces of the open-system tests (tests/test_open_host.py, tests/test_gpu_open.py): the vectorised problem is built
HERE, with numpy.kron, independently of the product's ``liouvillian()`` -- that function is a thing under test."""
import numpy as np

TOL_J = 1e-12
TOL_TAU = 1e-12


def tol_G(G):
    return 1e-10 * max(np.abs(G).max(), 1e-3)


def vec(rho):
    """column stacking: vec(A rho B) = (B^T (x) A) vec(rho)"""
    rho = np.asarray(rho)
    return np.swapaxes(rho, -1, -2).reshape(rho.shape[:-2] + (-1,))


def lindblad_rhs(H, cops, rho):
    """L(rho) written out in matrix form"""
    heff = H - 0.5j * sum((A.conj().T @ A for A in cops), np.zeros_like(H))
    out = -1j * (heff @ rho - rho @ heff.conj().T)
    for A in cops:
        out = out + A @ rho @ A.conj().T
    return out


def super_generator(H, cops):
    """i L as a d^2 x d^2 matrix (the 'H' of the vectorised problem): -i * super_generator @ vec(rho) = vec(L(rho))"""
    d = H.shape[0]
    eye = np.eye(d)
    heff = H - 0.5j * sum((A.conj().T @ A for A in cops), np.zeros_like(H))
    Lm = -1j * (np.kron(eye, heff) - np.kron(heff.conj(), eye))
    for A in cops:
        Lm = Lm + np.kron(A.conj(), A)
    return 1j * Lm


def vectorised(pr):
    """The closed-path problem of an open-system problem dict (H0 [K,d,d], Hc [L,d,d] or [K,L,d,d], cops [J,d,d] or
    [K,J,d,d], rho0, target): generators i L, control generators 1 (x) H_l - conj(H_l) (x) 1, vec'd states."""
    H0, Hc, cops = np.asarray(pr["H0"]), np.asarray(pr["Hc"]), np.asarray(pr["cops"])
    K, d = H0.shape[0], H0.shape[1]
    cops_k = (lambda k: list(cops[k])) if cops.ndim == 4 else (lambda k: list(cops))
    H0v = np.stack([super_generator(H0[k], cops_k(k)) for k in range(K)])
    ctrl = lambda H: super_generator(H, [])   # noqa: E731
    if Hc.ndim == 4:
        Hcv = np.stack([np.stack([ctrl(Hc[k, l]) for l in range(Hc.shape[1])]) for k in range(K)])
    else:
        Hcv = np.stack([ctrl(Hc[l]) for l in range(Hc.shape[0])])
    return dict(H0=H0v, Hc=Hcv, psi0=vec(pr["rho0"]), target=None if pr.get("target") is None else vec(pr["target"]))


def oracle(ref, pr, pulsevals, functional=0, weights=None, shape=None, tlist=None, want_parts=True):
    """grape_ref.evaluate on the vectorised problem.  The oracle has no shape argument: a_l = shape_ln eps_nl enters it as
    the pulse, and the chain rule d/d eps = shape * d/d a maps its gradient and tau_grads back."""
    v = vectorised(pr)
    tl = pr["tlist"] if tlist is None else tlist
    x = np.asarray(pulsevals, dtype=float)
    s = np.ones_like(x) if shape is None else np.asarray(shape, dtype=float).reshape(-1)
    J, G, tau, parts = ref.evaluate(v["H0"], v["Hc"], tl, s * x, v["psi0"], v["target"], weights, functional=functional,
                                    gradient_method=ref.GRADGEN, want_parts=True)
    L = len(x) // (len(tl) - 1)
    d = np.asarray(pr["H0"]).shape[1]
    K = np.asarray(pr["H0"]).shape[0]
    rhoT = np.swapaxes(parts["psiT"].reshape(K, d, d), -1, -2)
    return dict(J=J, G=s * G, tau=tau, rhoT=rhoT, tau_grads=parts["tau_grads"] * s.reshape(1, L, -1))
