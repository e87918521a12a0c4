"""A matrix-form reference of the open-system evaluation WITH a state running cost (grape_open_set_running_cost,
grape_open_backward_xi), on the conventions and problem dicts of tests/open_reference.py, generic over numpy.complex128 and
numpy.clongdouble.  It shares nothing with the kernels' adjoint trick: there is no backward sweep and no inhomogeneity.

    J = J_T + lambda_b J_b,      J_b = sum_k sum_{m=0}^{N_T} wq_m g_b(rho_k(t_m)),      dg_b = -2 Re <<xi | d rho>>
    wq_0 = (t_1 - t_0) / 2,   wq_m = (t_{m+1} - t_{m-1}) / 2,   wq_{N_T} = (t_{N_T} - t_{N_T-1}) / 2        (optimize.jl:727-750)

Every rho_k(t_m) is kept.  For every (n, l) the forward sensitivity S = d rho / d eps_nl is formed on interval n by the pair
series of open_reference.propagate and then carried through ALL later intervals with L alone, so that
    G_b[l][n] = sum_k sum_{m=n+1}^{N_T} wq_m (-2 Re <<xi_k(t_m) | S(t_m)>>),      G_T[l][n] = -2 Re sum_k conj(c_k) <<sigma_k | S(T)>>
which is O(N_T^2) series, fine at N_T = 3.  tau_grads[k][l][n] = conj(c_k) <<sigma_k | S(T)>> + lambda_b sum_m wq_m <<xi_k(t_m) | S(t_m)>>
is what the kernels' tau_grads hold, G = G_T + lambda_b G_b = -2 Re sum_k tau_grads.

The cost is the built-in family g_b = Re tr(D rho), xi = -D^dagger / 2 (D [d,d] shared or [K,d,d]), or the callbacks
g_b(rho, k, m) -> real and xi(rho, k, m) -> [d,d].
"""
import numpy as np

import open_helpers as oh
import open_reference as orf

TOL_JB = 1e-12

# deliberately wrong variants (tests of the tests only): what a subtly wrong kernel would compute
MUTATIONS = ("no_boundary", "xi_full", "no_rho_div", "wq_dt", "D_transposed", "D0_everywhere", "every_substep")


def trapezoid_weights(tl):
    N_T = len(tl) - 1
    wq = np.empty(N_T + 1, dtype=tl.dtype)
    wq[0] = (tl[1] - tl[0]) / 2
    wq[N_T] = (tl[N_T] - tl[N_T - 1]) / 2
    for m in range(1, N_T):
        wq[m] = (tl[m + 1] - tl[m - 1]) / 2
    return wq


def evaluate(pr, pulsevals, functional=0, D=None, lambda_b=1.0, g_b=None, xi=None, chi=None, weights=None, shape=None,
             tlist=None, dtype=np.complex128, theta=1.0, mutate=None):
    """dict(J, J_T, J_b, Jb_k [K], G, G_T, G_b [L*N_T], tau [K], rhoT [K,d,d], tau_grads [K,L,N_T], states [K,N_T+1,d,d],
    substeps [K,N_T], and the two parts base, run [K,L,N_T] of tau_grads = base + lambda_b run) in ``dtype``.  ``chi`` [K,d,d]: the caller's boundary matrices instead of c_k sigma_k (J_T and J are
    then None).  ``mutate``: one of MUTATIONS."""
    assert mutate is None or mutate in MUTATIONS
    assert (D is None) != (g_b is None and xi is None), "either D or the callbacks g_b and xi"
    rdt = orf._real(dtype)
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
    weights = pr.get("weights") if weights is None else weights
    lam = rdt(lambda_b)
    im = dtype(1j)
    wq = trapezoid_weights(tl)
    if mutate == "wq_dt":
        wq = np.concatenate([tl[1:] - tl[:-1], tl[-1:] - tl[-2:-1]])

    if D is not None:
        Dm = np.asarray(D, dtype=dtype)
        if mutate == "D_transposed":
            Dm = np.swapaxes(Dm, -1, -2)
        D_of = lambda k: Dm if Dm.ndim == 2 else Dm[0 if mutate == "D0_everywhere" else k]   # noqa: E731
        g_b = lambda rho, k, m: np.sum(D_of(k).T * rho).real                                   # noqa: E731  Re tr(D rho)
        xi = lambda rho, k, m: -orf._dag(D_of(k)) / (1 if mutate == "xi_full" else 2)          # noqa: E731

    states = np.empty((K, N_T + 1, d, d), dtype=dtype)
    msub = np.zeros((K, N_T), dtype=int)
    q = np.zeros((K, L, N_T, N_T + 1), dtype=dtype)      # <<xi_k(t_m) | d rho_k(t_m) / d eps_nl>>, m > n
    q_sub = np.zeros((K, L, N_T), dtype=dtype)            # "every_substep": what the extra additions inside cut intervals give
    sT = np.zeros((K, L, N_T, d, d), dtype=dtype)         # d rho_k(T) / d eps_nl
    for k in range(K):
        Hc, cops = orf._per_k(Hc_all, k, 3), orf._per_k(cops_all, k, 3)
        copsd = orf._dag(cops)
        AdA = sum((copsd[j] @ cops[j] for j in range(len(cops))), np.zeros((d, d), dtype=dtype))
        Dl = -im * Hc
        Dld = orf._dag(Dl)
        linds = []
        for n in range(N_T):
            H = H0[k] + sum((s[l, n] * eps[l, n]) * Hc[l] for l in range(L))
            M = -im * H - AdA / 2
            msub[k, n] = orf.substeps(M, cops, tl[n + 1] - tl[n], theta)

            def lind(X, M=M, Md=orf._dag(M)):
                out = M @ X + X @ Md
                for j in range(len(cops)):
                    out = out + cops[j] @ X @ copsd[j]
                return out
            linds.append(lind)
        # every rho_k(t_m)
        states[k, 0] = rho0[k]
        for n in range(N_T):
            Y = states[k, n][None]
            for _ in range(msub[k, n]):
                Y = orf._series(linds[n], Y, (tl[n + 1] - tl[n]) / msub[k, n], tol, None)
            states[k, n + 1] = Y[0]
        xis = [None] + [np.asarray(xi(states[k, m], k, m), dtype=dtype) for m in range(1, N_T + 1)]
        for n in range(N_T):
            def pair(Y, n=n, lind=linds[n]):
                out = lind(Y)
                for l in range(L):
                    out[1 + l] = out[1 + l] + s[l, n] * (Dl[l] @ Y[0] + Y[0] @ Dld[l])
                return out
            Y = np.concatenate([states[k, n][None], np.zeros((L, d, d), dtype=dtype)])
            for _ in range(msub[k, n]):
                Y = orf._series(pair, Y, (tl[n + 1] - tl[n]) / msub[k, n], tol, None)
            S = Y[1:]
            q[k, :, n, n + 1] = np.sum(np.conj(xis[n + 1]) * S, axis=(-2, -1))
            for m in range(n + 1, N_T):       # through interval m, to t_{m+1}
                for j in range(msub[k, m]):
                    if j > 0:   # a wrong kernel adds xi_k(t_m) behind EVERY sub-step of interval m, not only behind the last one
                        q_sub[k, :, n] += wq[m] * np.sum(np.conj(xis[m]) * S, axis=(-2, -1))
                    S = orf._series(linds[m], S, (tl[m + 1] - tl[m]) / msub[k, m], tol, None)
                q[k, :, n, m + 1] = np.sum(np.conj(xis[m + 1]) * S, axis=(-2, -1))
            sT[k, :, n] = S

    rhoT = states[:, N_T]
    gb = np.array([[g_b(states[k, m], k, m) for m in range(N_T + 1)] for k in range(K)], dtype=rdt)
    Jb_k = gb @ wq
    J_b = np.sum(Jb_k)
    if chi is None:
        target = np.asarray(pr["target"], dtype=dtype)
        tau = np.sum(np.conj(target) * rhoT, axis=(-2, -1))
        J_T, c = orf.functional_values(tau, weights, functional)
        B = c[:, None, None] * target
    else:
        tau, J_T = None, None
        B = np.asarray(chi, dtype=dtype)
    base = np.sum(np.conj(B)[:, None, None] * sT, axis=(-2, -1))                # <<chi_k(T) | d rho_k(T) / d eps_nl>>  [K,L,N_T]
    wts = np.array(wq, copy=True)
    if mutate == "no_boundary":
        wts[N_T] = 0
    run = np.sum(q * wts, axis=-1)                                              # [K,L,N_T]
    if mutate == "no_rho_div":     # the kernel scales tau_grads by rho_k = ||chi_k(T)||_F: a term it forgot to divide keeps the factor
        rho_k = orf._fro(B + lam * wq[N_T] * np.stack([np.asarray(xi(states[k, N_T], k, N_T), dtype=dtype) for k in range(K)]))
        interior = np.sum(q[..., :N_T] * wts[:N_T], axis=-1)
        run = run + (rho_k[:, None, None] - 1) * interior
    if mutate == "every_substep":
        run = run + q_sub
    tg = base + lam * run
    G_T = -2 * np.sum(base, axis=0).real
    G_b = -2 * np.sum(run, axis=0).real
    G = -2 * np.sum(tg, axis=0).real
    return dict(J=None if J_T is None else J_T + lam * J_b, J_T=J_T, J_b=J_b, Jb_k=Jb_k, G=G.reshape(-1), G_T=G_T.reshape(-1),
                G_b=G_b.reshape(-1), tau=tau, rhoT=rhoT, tau_grads=tg, states=states, substeps=msub, base=base, run=run)


def with_lambda(want, lambda_b):
    """the outputs of ``evaluate`` (without a mutation) at another lambda_b: J, G and tau_grads are linear in it"""
    out = dict(want)
    out["tau_grads"] = want["base"] + lambda_b * want["run"]
    out["G"] = want["G_T"] + lambda_b * want["G_b"]
    out["J"] = None if want["J_T"] is None else want["J_T"] + lambda_b * want["J_b"]
    return out


def hermitian_D(seed, d, K=None):
    """a random complex Hermitian D of unit 2-norm ([d,d]), or one per trajectory ([K,d,d]), from the project's generator"""
    from grape_jl_amd import synth
    out = []
    for k in range(1 if K is None else K):
        D = synth.gue(synth.subseed(seed, 8200 + k), d)
        out.append(D / np.linalg.norm(D, 2))
    return out[0] if K is None else np.stack(out)


def lambda_from(want):
    """the power of two nearest ||G_T||_inf / ||G_b||_inf: both parts of the gradient the same size (the reference alone decides)"""
    return float(2.0 ** np.round(np.log2(float(np.abs(want["G_T"]).max()) / float(np.abs(want["G_b"]).max()))))


def assert_order_one(want, lambda_b):
    """the conditions ON THE REFERENCE ALONE under which ||dG||_inf <= 1e-10 ||G||_inf is relative for both parts"""
    fig = dict(tau_min=float(np.abs(want["tau"]).min()), GT=float(np.abs(want["G_T"]).max()),
               lGb=float(lambda_b * np.abs(want["G_b"]).max()), G=float(np.abs(want["G"]).max()), lambda_b=lambda_b)
    print(fig)
    assert fig["tau_min"] >= 0.1 and fig["GT"] >= 1e-3 and fig["lGb"] >= 1e-3 and fig["G"] >= 1e-3
    return fig


def assert_runcost_agrees(got, want, label=""):
    """THE comparison of the running-cost tests: open_helpers.assert_open_agrees on every output ``want`` holds of J, tau, G,
    rhoT, tau_grads, plus |dJ_b| <= 1e-12 where both sides hold J_b"""
    keys = ("J", "tau", "G", "rhoT", "tau_grads")
    fig = oh.assert_open_agrees({k: got[k] for k in keys if k in got and got[k] is not None},
                                {k: want[k] for k in keys if k in want and want[k] is not None and k in got}, label)
    if "J_b" in got and "J_b" in want:
        fig["dJb"] = float(abs(got["J_b"] - want["J_b"]))
        print(label, dict(dJb=fig["dJb"]))
        assert fig["dJb"] <= TOL_JB
    return fig
