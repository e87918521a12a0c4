"""Reference of the split-phase Hessian-vector products on open-system handles (grape_open_hvp_forward / _backward /
_backward_chi) in plain numpy, generic over numpy.complex128 and numpy.clongdouble, with the boundary left to
the caller, and the shared comparison of its tests (tests/test_open_hvp_split_reference.py proves both;
tests/test_gpu_open_hvp_split.py uses them).

``evaluate_chi``: FORWARD OVER FORWARD in matrix form, restated from open_reference's helpers -- the stack
(rho, rho'_v, sigma_nl, sigma'_nl,v) of open_hvp_reference.evaluate (same generator, same sub-steps, same stopping rule) is
carried to T, and there a callback
    boundary(rho(T) [K, d, d], rho'(T) [nv, K, d, d]) -> (J, chi [K, d, d], chi' [nv, K, d, d])
supplies J, chi_k(T) = -dJ/d<<rho_k(T)| and its derivative along every direction.  With i = (n, l)
    G_i      = -2 Re sum_k <<chi_k | sigma_i>>
    (H v)_i  = -2 Re sum_k (<<chi'_k,v | sigma_i>> + <<chi_k | sigma'_i,v>>).
No targets are needed (dtau is returned where the problem has them).

``hilbert_schmidt``: the test functional J = sum_k w_k ||rho_k(T) - sigma_k||_F^2 / (2 K), chi_k = -w_k (rho_k(T) - sigma_k) / (2 K),
chi'_k = -w_k rho'_k(T) / (2 K), sigma_k the caller's.  ``builtin``: the three functionals of the library written as a boundary.
"""
import numpy as np

import open_hvp_reference as ohr
import open_reference as orf

SM, SS, RE = 0, 1, 2
WRONG = ("drop_rho_prime",)


def inner(A, B):
    """<<A|B>> = tr(A^dagger B) over the last two axes"""
    return np.sum(np.conj(A) * B, axis=(-2, -1))


def stack_to_T(pr, pulsevals, V, dtype=np.complex128, theta=1.0, tlist=None, shape=None, weights=None, wrong=None):
    """dict(rhoT [K,d,d], drhoT [nv,K,d,d], S [K,N_T,L,d,d] = d rho_k(T) / d eps_nl, SP [K,N_T,L,nv,d,d] its derivative along v,
    plus the set-up) -- the propagation of open_hvp_reference.evaluate, term for term.  ``wrong="drop_rho_prime"`` leaves the
    source D_l rho'_v out of sigma' (the mutation tests of the shared comparison)."""
    assert wrong is None or wrong in WRONG
    q = ohr._setup(dict(pr, target=pr["target"] if pr.get("target") is not None else np.zeros_like(pr["rho0"])), pulsevals, V, dtype,
                   tlist, shape, weights)
    rdt, K, d, L, N_T, s, eps, Vs = q["rdt"], q["K"], q["d"], q["L"], q["N_T"], q["s"], q["eps"], q["V"]
    nv = len(Vs)
    tol = rdt(1e-24) if rdt is np.longdouble else rdt(1e-18)
    im = dtype(1j)
    rhoT = np.empty((K, d, d), dtype=dtype)
    drhoT = np.empty((nv, K, d, d), dtype=dtype)
    ST = np.empty((K, N_T, L, d, d), dtype=dtype)
    SPT = np.empty((K, N_T, L, nv, d, d), dtype=dtype)
    for k in range(K):
        Hc, cops = orf._per_k(q["Hc"], k, 3), orf._per_k(q["cops"], k, 3)
        copsd = orf._dag(cops)
        AdA = sum((copsd[j] @ cops[j] for j in range(len(cops))), np.zeros((d, d), dtype=dtype))
        D = -im * Hc
        Dd = orf._dag(D)
        R = np.concatenate([q["rho0"][k][None], np.zeros((nv, d, d), dtype=dtype)])      # rho, rho'_v
        S = np.zeros((0, d, d), dtype=dtype)                                               # sigma_(m,l), m <= n
        SP = np.zeros((0, nv, d, d), dtype=dtype)                                          # sigma'_(m,l),v
        for n in range(N_T):
            H = q["H0"][k] + sum((s[l, n] * eps[l, n]) * Hc[l] for l in range(L))
            M = -im * H - AdA / 2
            Md = orf._dag(M)
            Bv = np.stack([sum((Vs[v, l, n] * s[l, n]) * D[l] for l in range(L)) for v in range(nv)])
            Bvd = orf._dag(Bv)
            S = np.concatenate([S, np.zeros((L, d, d), dtype=dtype)])
            SP = np.concatenate([SP, np.zeros((L, nv, d, d), dtype=dtype)])
            ns, first = len(S), n * L

            def lind(X):
                out = M @ X + X @ Md
                for j in range(len(cops)):
                    out = out + cops[j] @ X @ copsd[j]
                return out

            def gen(Y):
                R_, S_ = Y[:1 + nv], Y[1 + nv:1 + nv + ns]
                out = lind(Y)
                oR, oS, oSP = out[:1 + nv], out[1 + nv:1 + nv + ns], out[1 + nv + ns:].reshape(ns, nv, d, d)
                oR[1:] += Bv @ R_[0] + R_[0] @ Bvd
                oSP += Bv[None] @ S_[:, None] + S_[:, None] @ Bvd[None]
                for l in range(L):
                    oS[first + l] += s[l, n] * (D[l] @ R_[0] + R_[0] @ Dd[l])
                    if wrong != "drop_rho_prime":
                        oSP[first + l] += s[l, n] * (D[l] @ R_[1:] + R_[1:] @ Dd[l])
                return out

            dt = q["tl"][n + 1] - q["tl"][n]
            m = orf.substeps(M, cops, dt, theta)
            Y = np.concatenate([R, S, SP.reshape(ns * nv, d, d)])
            for _ in range(m):
                Y = orf._series(gen, Y, dt / m, tol, None)
            R, S, SP = Y[:1 + nv], Y[1 + nv:1 + nv + ns], Y[1 + nv + ns:].reshape(ns, nv, d, d)
        rhoT[k], drhoT[:, k] = R[0], R[1:]
        ST[k], SPT[k] = S.reshape(N_T, L, d, d), SP.reshape(N_T, L, nv, d, d)
    return dict(q=q, rhoT=rhoT, drhoT=drhoT, S=ST, SP=SPT)


def contract(chi, dchi, S, SP):
    """(G [L*N_T], Hv [nv, L*N_T], Hv with chi' = 0) of a boundary (chi [K,d,d], chi' [nv,K,d,d]) on the stack at T"""
    K, N_T, L, nv = SP.shape[:4]
    G = -2 * np.sum(inner(chi[:, None, None], S), axis=0).real                                          # [n][l]
    from_chi = -2 * np.sum(inner(chi[:, None, None, None], SP), axis=0).real                             # [n][l][v]
    from_dchi = -2 * np.sum(inner(np.moveaxis(dchi, 0, 1)[:, None, None], S[:, :, :, None]), axis=0).real
    order = lambda X: np.moveaxis(X, -1, 0).transpose(0, 2, 1).reshape(nv, L * N_T)   # noqa: E731   [v][l][n]
    return G.T.reshape(-1), order(from_chi + from_dchi), order(from_chi)


def evaluate_chi(pr, pulsevals, V, boundary, dtype=np.complex128, theta=1.0, tlist=None, shape=None, weights=None, wrong=None,
                 want_parts=False):
    """dict(J, G [L*N_T], Hv [nv, L*N_T] (or [L*N_T] for a 1-D V), Hv_chi0 (the same with chi' = 0), rhoT [K,d,d],
    drhoT [nv,K,d,d], dtau [nv,K] or None without targets, chi, dchi) of a caller's boundary, in the real type of ``dtype``."""
    st = stack_to_T(pr, pulsevals, V, dtype, theta, tlist, shape, weights, wrong)
    q = st["q"]
    J, chi, dchi = boundary(st["rhoT"], st["drhoT"])
    chi, dchi = np.asarray(chi, dtype=dtype), np.asarray(dchi, dtype=dtype)
    G, Hv, Hv0 = contract(chi, dchi, st["S"], st["SP"])
    dtau = None if pr.get("target") is None else inner(np.asarray(pr["target"], dtype=dtype)[None], st["drhoT"])
    one = (lambda X: X[0]) if q["one"] else (lambda X: X)
    out = dict(J=J, G=G, Hv=one(Hv), Hv_chi0=one(Hv0), rhoT=st["rhoT"], drhoT=st["drhoT"], dtau=dtau, chi=chi, dchi=dchi)
    if want_parts:
        out.update(S=st["S"], SP=st["SP"])
    return out


def hilbert_schmidt(sigma, weights=None, K_total=None):
    """the boundary callback of J = sum_k w_k ||rho_k(T) - sigma_k||_F^2 / (2 K)"""
    def boundary(rhoT, drhoT):
        dtype = rhoT.dtype
        K = len(rhoT) if K_total is None else K_total
        w = np.ones(len(rhoT), dtype=rhoT.real.dtype) if weights is None else np.asarray(weights, dtype=rhoT.real.dtype)
        diff = rhoT - np.asarray(sigma, dtype=dtype)
        J = np.sum(w * inner(diff, diff).real) / (2 * K)
        c = (-w / (2 * K))[:, None, None]
        return J, c * diff, c[None] * drhoT
    return boundary


def builtin(target, functional, weights=None):
    """the library's three functionals written as a boundary: chi_k = c_k sigma_k, chi'_k = c'_k sigma_k (include/grape_hip.h)"""
    def boundary(rhoT, drhoT):
        dtype = rhoT.dtype
        K = len(rhoT)
        sg = np.asarray(target, dtype=dtype)
        w = np.ones(K, dtype=rhoT.real.dtype) if weights is None else np.asarray(weights, dtype=rhoT.real.dtype)
        tau, dtau = inner(sg, rhoT), inner(sg[None], drhoT)
        J, c = orf.functional_values(tau, w, functional)
        if functional == SM:
            dc = w[None, :] * np.sum(w * dtau, axis=1)[:, None] / K ** 2
        elif functional == SS:
            dc = w[None, :] * dtau / K
        else:
            dc = np.zeros_like(dtau)
        return J, np.asarray(c, dtype=dtype)[:, None, None] * sg, dc[:, :, None, None] * sg[None]
    return boundary


def assert_reference_conditions(want):
    """the conditions ON THE REFERENCE ALONE under which the bound below is relative and a dropped chi' cannot pass"""
    G, Hv, Hv0 = (np.asarray(want[key], dtype=float) for key in ("G", "Hv", "Hv_chi0"))
    fig = dict(G_max=float(np.abs(G).max()), Hv_max=float(np.abs(Hv).max()), dchi_part=float(np.abs(Hv - Hv0).max()))
    print(fig)
    assert fig["G_max"] >= 1e-3
    assert fig["Hv_max"] >= 1e-3
    assert fig["dchi_part"] >= 1e-2 * fig["Hv_max"]
    return fig


def assert_open_hvp_split_agrees(got, want, label=""):
    """THE comparison of the caller's route: ``want`` is evaluate_chi's dict, ``got`` the H v under test.
    ||got - want||_inf <= 1e-10 max(||want||_inf, 1e-3) (the project's tol_hv) after the conditions on the reference alone."""
    assert_reference_conditions(want)
    ref = np.asarray(want["Hv"], dtype=float)
    got = np.asarray(got, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got))
    dev, tol = float(np.abs(got - ref).max()), ohr.tol_hv(ref)
    print(label, dict(dHv=dev, tol=tol, rel=dev / float(np.abs(ref).max())))
    assert dev <= tol, (label, dev, tol)
    return dev


_CACHE = {}


def reference_of(name, cases, nv=2):
    """(problem, V [nv, L*N_T], sigma [K,d,d], evaluate_chi(..., hilbert_schmidt(sigma))) of a named case spec of
    open_time_reference.build_case: computed once, shared, never modified.  sigma is the target of the case (a state the pulse
    ``factor`` x reaches, so that rho(T) - sigma is neither zero nor of order one in every entry); ``no_target`` removes the
    target from the problem afterwards -- the functional keeps its sigma."""
    import open_time_reference as otr
    if name not in _CACHE:
        c = cases[name]
        pr = otr.build_case(c)
        V = ohr.directions(c.get("seed", 0) + 17 * c["d"], c.get("nv", nv), pr["pulsevals"].size)
        sigma = np.array(pr["target"])
        if c.get("no_target"):
            pr = dict(pr, target=None)
        _CACHE[name] = (pr, V, sigma, evaluate_chi(pr, pr["pulsevals"], V, hilbert_schmidt(sigma, pr.get("weights"))))
    return _CACHE[name]
