"""Reference of grape_open_hessian (the exact Hessian of J as a matrix on an open-system handle) in plain numpy, and the shared
comparison of its tests (tests/test_open_hessian_reference.py proves both against the forward-over-forward reference of
tests/open_hvp_reference.py, tests/test_gpu_open_hessian.py uses them).

ADJOINT FORM on the stored states, complex128, every series summed until ||term||_F <= 1e-18 ||sum||_F for every member, on
m = open_reference.substeps(...) equal sub-steps (theta = 1, the reference's own rule).  With <<Y|X>> = tr(Y^dagger X),
    L_n(X) = M X + X M^dagger + sum_j A_j X A_j^dagger,   E_n = exp(dt_n L_n): t_n -> t_{n+1},
    D_nl(X) = s_ln (D_l X + X D_l^dagger),   D_l = -i H_l,
per trajectory
    theta_k(T) = sigma_k,   theta_k(t_n) = E_n^dagger theta_k(t_{n+1})          the bare target chain
    a_(n,l)    = DE_n[D_nl] rho_k(t_n)                                          lives at t_{n+1}
    beta_(n,l) = DE_n[D_nl]^dagger theta_k(t_{n+1})                             lives at t_n
    T_k,p      = d tau_k / d eps_p = <<beta_p | rho_k(t_n)>>                    p = (n, l)
    S_k,pq     = <<beta_(n,l) | E_{n-1} ... E_{m+1} a_(m,l')>>                  m < n
               = <<theta_k(t_{n+1}) | D^2E_n[D_nl, D_nl'] rho_k(t_n)>>          m = n;     symmetric in p <-> q
    G_p  = -2 Re sum_k conj(c_k) T_k,p                                          chi_k(T) = c_k sigma_k (include/grape_hip.h)
    H_pq = -2 Re sum_k [ conj(c_k) S_k,pq + conj(d_q c_k) T_k,p ]
           sm: d_q c_k = w_k F_q / K_total^2, F_q = sum_j w_j T_j,q;   ss: d_q c_k = w_k T_k,q / K_total;   re: 0
The first derivatives are the off-diagonal blocks of the series of the block generators [[L, D], [0, L]] (forward) and its
adjoint; the second derivative comes from the three-level block generator of the adjoint side, whose last member
    beta2' = L^dagger beta2 + D_nl^dagger beta_l' + D_nl'^dagger beta_l
gives D^2E_n[D_nl, D_nl']^dagger theta (for l = l' with the factor 2 of the second derivative).  The result is indexed like
G: p = l * N_T + n.

``wrong=`` switches ONE deliberate mistake on (the refusal tests of the shared comparison).
"""
import numpy as np

import open_hvp_reference as ohr
import open_reference as orf

SM, SS, RE = 0, 1, 2
WRONG = ("drop_diagonal_blocks", "drop_boundary", "fan_one_interval_too_many", "no_dissipator_in_columns", "k_for_k_total",
         "ignore_last_weight")
TOL = 1e-18


def tol_open_hessian(H):
    """the project's bar for H v (open_hvp_reference.tol_hv) applied to the entries of H"""
    return 1e-10 * max(float(np.abs(np.asarray(H, dtype=float)).max()), 1e-3)


def assert_open_hessian_agrees(got, want, label=""):
    """THE comparison of the open Hessian tests: ``want`` is the reference's dict (tau, G, H), ``got`` the matrix under test.
    The conditions on the reference alone first (open_hvp_reference.assert_order_one on tau, G, H), then
    ||got - want||_inf <= 1e-10 max(||want||_inf, 1e-3) over all entries."""
    ohr.assert_order_one(dict(tau=want["tau"], G=want["G"], Hv=want["H"]))
    ref = np.asarray(want["H"], dtype=float)
    got = np.asarray(got, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got))
    dev, tol = float(np.abs(got - ref).max()), tol_open_hessian(ref)
    print(label, dict(dH=dev, tol=tol, rel=dev / float(np.abs(ref).max())))
    assert dev <= tol, (label, dev, tol)
    return dev


def evaluate(pr, pulsevals, functional=0, K_total=None, wrong=None, theta=1.0):
    """dict(J, G [L*N_T], tau [K], H [L*N_T, L*N_T]) at the pulses ``pulsevals`` (control-major) of the problem dicts of the
    open-system tests.  ``K_total``: the trajectories of the whole problem (default: those of ``pr``)."""
    assert wrong is None or wrong in WRONG
    dtype = np.complex128
    q = ohr._setup(pr, pulsevals, np.zeros(np.size(pulsevals)), dtype)
    K, d, L, N_T, s, eps = q["K"], q["d"], q["L"], q["N_T"], q["s"], q["eps"]
    w = q["w"].copy()
    if wrong == "ignore_last_weight":
        w[-1] = 1.0
    Kt = float(K if K_total is None or wrong == "k_for_k_total" else K_total)
    dts = np.diff(q["tl"])
    P = L * N_T
    pairs = [(l, l2) for l in range(L) for l2 in range(l + 1)]

    T = np.zeros((K, N_T, L), dtype)                   # T_k,(n,l)
    Sm = np.zeros((K, N_T, L, N_T, L), dtype)          # S_k,(n,l)(m,l')
    tau = np.zeros(K, dtype)
    for k in range(K):
        Hc, cops = orf._per_k(q["Hc"], k, 3), orf._per_k(q["cops"], k, 3)
        copsd = orf._dag(cops)
        AdA = sum((copsd[j] @ cops[j] for j in range(len(cops))), np.zeros((d, d), dtype=dtype))
        D = -1j * Hc
        Dd = orf._dag(D)
        gens = []
        for n in range(N_T):
            M = -1j * (q["H0"][k] + sum((s[l, n] * eps[l, n]) * Hc[l] for l in range(L))) - AdA / 2
            gens.append((M, orf._dag(M), orf.substeps(M, cops, dts[n], theta)))

        def lind(X, n, diss=True):
            M, Md, _ = gens[n]
            out = M @ X + X @ Md
            if diss:
                for j in range(len(cops)):
                    out = out + cops[j] @ X @ copsd[j]
            return out

        def adj(Y, n):
            M, Md, _ = gens[n]
            out = Md @ Y + Y @ M
            for j in range(len(cops)):
                out = out + copsd[j] @ Y @ cops[j]
            return out

        def run(gen, Y, n):
            m = gens[n][2]
            for _ in range(m):
                Y = orf._series(gen, Y, dts[n] / m, TOL, None)
            return Y

        # forward: the stored states and the seeds a_(n,l)
        rho = [q["rho0"][k]]
        a = []
        for n in range(N_T):
            def fwd(Y, n=n):
                out = lind(Y, n)
                for l in range(L):
                    out[1 + l] += s[l, n] * (D[l] @ Y[0] + Y[0] @ Dd[l])
                return out

            Y = run(fwd, np.concatenate([rho[n][None], np.zeros((L, d, d), dtype)]), n)
            rho.append(Y[0])
            a.append(Y[1:])
        tau[k] = np.sum(np.conj(q["target"][k]) * rho[-1])
        # backward from the bare target: beta_(n,l), T, the diagonal blocks
        theta_k = q["target"][k]
        beta = [None] * N_T
        for n in range(N_T - 1, -1, -1):
            def bwd(Y, n=n):
                out = adj(Y, n)
                for l in range(L):
                    out[1 + l] += s[l, n] * (Dd[l] @ Y[0] + Y[0] @ D[l])
                for i, (l, l2) in enumerate(pairs):
                    out[1 + L + i] += s[l, n] * (Dd[l] @ Y[1 + l2] + Y[1 + l2] @ D[l]) + s[l2, n] * (Dd[l2] @ Y[1 + l] + Y[1 + l] @ D[l2])
                return out

            Y = run(bwd, np.concatenate([theta_k[None], np.zeros((L + len(pairs), d, d), dtype)]), n)
            theta_k, beta[n] = Y[0], Y[1:1 + L]
            T[k, n] = np.sum(np.conj(beta[n]) * rho[n][None], axis=(-2, -1))
            if wrong != "drop_diagonal_blocks":
                for i, (l, l2) in enumerate(pairs):
                    Sm[k, n, l, n, l2] = Sm[k, n, l2, n, l] = np.sum(np.conj(Y[1 + L + i]) * rho[n])
        # the fan: the columns a_(m, .) are carried forwards and overlapped with beta_(n, .) at every later grid point
        X = np.zeros((0, d, d), dtype)
        for n in range(1, N_T):
            born = a[n - 1]
            if wrong == "fan_one_interval_too_many":
                born = run(lambda Y, n=n: lind(Y, n), born, n)
            X = np.concatenate([X, born])                                      # interval-major: q = m L + l'
            ov = np.einsum("lij,qij->lq", np.conj(beta[n]), X)                  # <<beta_(n,l) | X_q>>, q < n L
            Sm[k, n].reshape(L, P)[:, :n * L] = ov
            Sm[k].reshape(P, N_T, L)[:n * L, n, :] = ov.T
            if n + 1 < N_T:
                X = run(lambda Y, n=n: lind(Y, n, diss=wrong != "no_dissipator_in_columns"), X, n)

    f = np.sum(w * tau)
    J = [1.0 - abs(f) ** 2 / Kt ** 2, 1.0 - np.sum(w * np.abs(tau) ** 2) / Kt, 1.0 - np.real(f) / Kt][functional]
    c = [w * f / Kt ** 2, w * tau / Kt, w / (2.0 * Kt) + 0j * tau][functional]
    Tp, Sp = T.reshape(K, P), Sm.reshape(K, P, P)      # interval-major: (n, l) -> n L + l
    G = -2.0 * np.real(np.einsum("k,kp->p", c.conj(), Tp))
    Hm = np.real(np.einsum("k,kpq->pq", c.conj(), Sp))
    if wrong != "drop_boundary":
        if functional == SM:
            F = np.einsum("k,kq->q", w, Tp)
            dc = w[:, None] * F[None, :] / Kt ** 2      # [k, q]
        elif functional == SS:
            dc = w[:, None] * Tp / Kt
        else:
            dc = np.zeros((K, P), dtype)
        Hm = Hm + np.real(np.einsum("kq,kp->pq", dc.conj(), Tp))
    Hm = -2.0 * Hm
    perm = np.array([n * L + l for l in range(L) for n in range(N_T)])         # (n, l) -> p = l N_T + n
    return dict(J=float(J), G=G[perm], tau=tau, H=Hm[np.ix_(perm, perm)])


_CACHE = {}


def reference_of(name, cases):
    """(problem, evaluate(...)) of a named case spec of open_time_reference.build_case: computed once, shared, never modified"""
    import open_time_reference as otr
    if name not in _CACHE:
        pr = otr.build_case(cases[name])
        _CACHE[name] = (pr, evaluate(pr, pr["pulsevals"], pr["functional"]))
    return _CACHE[name]
