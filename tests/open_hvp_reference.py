"""Reference of grape_open_hvp (exact Hessian-vector products of J on an open-system handle) in plain numpy, generic over
numpy.complex128 and numpy.clongdouble like open_reference.py, the shared comparison of its tests, and a numpy transcription of
the kernels' block recursion (tests/test_open_hvp_reference.py proves all three; tests/test_gpu_open_hvp.py uses them).

``evaluate``: FORWARD OVER FORWARD, in matrix form -- nothing of the kernels' adjoint recursion.  With
    L(X) = M X + X M^dagger + sum_j A_j X A_j^dagger,   D_l(X) = s_ln (D_l X + X D_l^dagger),   B_v(X) = sum_l v_nl D_l(X),   D_l = -i H_l
the stack (rho, rho'_v, sigma_nl, sigma'_nl,v) obeys on interval m
    d rho / dt       = L rho
    d rho'_v / dt    = L rho'_v + B_v rho
    d sigma_nl / dt  = L sigma_nl + [m == n] D_l rho                                  (sigma_nl = d rho / d eps_nl, zero before t_n)
    d sigma'_nl,v/dt = L sigma'_nl,v + B_v sigma_nl + [m == n] D_l rho'_v             (the mixed second derivative)
and is summed as the Taylor series of that (linear) generator on m = open_reference.substeps(...) equal sub-steps (theta <= 1,
the reference's own rule), every series until ||term||_F <= tol ||sum||_F for every member: tol = 1e-18 / 1e-24.  At T
    tau = <<sigma_k|rho>>, tau'_v, tau_,i = <<sigma_k|sigma_i>>, tau_,iv = <<sigma_k|sigma'_i,v>>        (i = (n, l)), f = sum_k w_k tau_k
    sm: G_i = -2 Re(conj(f) f_,i) / K^2         (Hv)_i = -2 Re(conj(f'_v) f_,i + conj(f) f_,iv) / K^2
    ss: G_i = -2 sum_k w_k Re(conj(tau) tau_,i) / K     (Hv)_i = -2 sum_k w_k Re(conj(tau'_v) tau_,i + conj(tau) tau_,iv) / K
    re: G_i = -Re f_,i / K                      (Hv)_i = -Re f_,iv / K

``block_recursion``: what csrc/grape_lindblad_hvp.hip.h does, in numpy -- the adjoint form on the stored states, with sub-steps
by a rule of the kernels' kind (beta from 2-norms, theta = 3) and all chains carried over between sub-steps.  ``wrong=`` switches
ONE deliberate mistake on (the refusal tests of the shared comparison).
"""
import numpy as np

import open_reference as orf

SM, SS, RE = 0, 1, 2
WRONG = ("drop_Bdag_p", "zero_chi_prime", "drop_rho_prime", "no_dissipator_in_primed", "swap_B_Bdag", "shape_shift", "ignore_last_weight")


def tol_hv(Hv):
    """the project's gradient tolerance applied to H v (tests/open_helpers.py: tol_G)"""
    return 1e-10 * max(float(np.abs(np.asarray(Hv, dtype=float)).max()), 1e-3)


def assert_order_one(want):
    """the conditions on the REFERENCE alone under which the bound of assert_open_hvp_agrees is relative, never its floor"""
    fig = dict(tau_min=float(np.abs(np.asarray(want["tau"], dtype=complex)).min()),
               G_max=float(np.abs(np.asarray(want["G"], dtype=float)).max()),
               Hv_max=float(np.abs(np.asarray(want["Hv"], dtype=float)).max()))
    print(fig)
    assert fig["tau_min"] >= 0.1
    assert fig["G_max"] >= 1e-3
    assert fig["Hv_max"] >= 1e-3
    return fig


def assert_open_hvp_agrees(got, want, label=""):
    """THE comparison of the open H v tests: ``want`` is the reference's dict (tau, G, Hv), ``got`` the H v under test.
    ||got - want||_inf <= 1e-10 max(||want||_inf, 1e-3) after the conditions on the reference alone."""
    assert_order_one(want)
    ref = np.asarray(want["Hv"], dtype=float)
    got = np.asarray(got, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got))
    dev, tol = float(np.abs(got - ref).max()), tol_hv(ref)
    print(label, dict(dHv=dev, tol=tol, rel=dev / float(np.abs(ref).max())))
    assert dev <= tol, (label, dev, tol)
    return dev


def _setup(pr, pulsevals, V, dtype, tlist=None, shape=None, weights=None):
    rdt = orf._real(dtype)
    H0 = np.asarray(pr["H0"], dtype=dtype)
    K, d = H0.shape[0], H0.shape[1]
    Hc = np.asarray(pr["Hc"], dtype=dtype)
    L = Hc.shape[-3]
    cops = np.zeros((0, d, d), dtype=dtype) if pr.get("cops") is None or np.size(pr["cops"]) == 0 else np.asarray(pr["cops"], dtype=dtype)
    tl = np.asarray(pr["tlist"] if tlist is None else tlist, dtype=rdt)
    N_T = len(tl) - 1
    shape = pr.get("shape") if shape is None else shape
    s = np.ones((L, N_T), dtype=rdt) if shape is None else np.asarray(shape, dtype=rdt).reshape(L, N_T)
    weights = pr.get("weights") if weights is None else weights
    w = np.ones(K, dtype=rdt) if weights is None else np.array(weights, dtype=rdt)
    Vs = np.asarray(V, dtype=rdt)
    one = Vs.ndim == 1
    return dict(rdt=rdt, H0=H0, K=K, d=d, Hc=Hc, L=L, cops=cops, tl=tl, N_T=N_T, s=s, w=w, eps=np.asarray(pulsevals, dtype=rdt).reshape(L, N_T),
                V=Vs.reshape(-1, L, N_T), one=one, rho0=np.asarray(pr["rho0"], dtype=dtype), target=np.asarray(pr["target"], dtype=dtype))


def evaluate(pr, pulsevals, V, functional=0, dtype=np.complex128, theta=1.0, tlist=None, shape=None, weights=None):
    """dict(J, G [L*N_T], tau [K], Hv [nv, L*N_T] or [L*N_T] for a 1-D V, dtau [nv, K]) at the pulses ``pulsevals`` (control-major)
    of the problem dicts of the open-system tests (open_reference.evaluate), in the real type of ``dtype``."""
    q = _setup(pr, pulsevals, V, dtype, tlist, shape, weights)
    rdt, K, d, L, N_T, s, w, eps, Vs = q["rdt"], q["K"], q["d"], q["L"], q["N_T"], q["s"], q["w"], q["eps"], q["V"]
    nv = len(Vs)
    tol = rdt(1e-24) if rdt is np.longdouble else rdt(1e-18)
    im = dtype(1j)
    tau = np.empty(K, dtype=dtype)
    dtau = np.empty((nv, K), dtype=dtype)
    tau_i = np.empty((K, N_T, L), dtype=dtype)
    tau_iv = np.empty((K, N_T, L, nv), dtype=dtype)
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
                R_, S_, SP_ = Y[:1 + nv], Y[1 + nv:1 + nv + ns], Y[1 + nv + ns:].reshape(ns, nv, d, d)
                out = lind(Y)
                oR, oS, oSP = out[:1 + nv], out[1 + nv:1 + nv + ns], out[1 + nv + ns:].reshape(ns, nv, d, d)
                oR[1:] += Bv @ R_[0] + R_[0] @ Bvd
                oSP += Bv[None] @ S_[:, None] + S_[:, None] @ Bvd[None]
                for l in range(L):
                    oS[first + l] += s[l, n] * (D[l] @ R_[0] + R_[0] @ Dd[l])
                    oSP[first + l] += s[l, n] * (D[l] @ R_[1:] + R_[1:] @ Dd[l])
                return out

            dt = q["tl"][n + 1] - q["tl"][n]
            m = orf.substeps(M, cops, dt, theta)
            Y = np.concatenate([R, S, SP.reshape(ns * nv, d, d)])
            for _ in range(m):
                Y = orf._series(gen, Y, dt / m, tol, None)
            R, S, SP = Y[:1 + nv], Y[1 + nv:1 + nv + ns], Y[1 + nv + ns:].reshape(ns, nv, d, d)
        tc = np.conj(q["target"][k])
        tau[k] = np.sum(tc * R[0])
        dtau[:, k] = np.sum(tc * R[1:], axis=(-2, -1))
        tau_i[k] = np.sum(tc * S, axis=(-2, -1)).reshape(N_T, L)
        tau_iv[k] = np.sum(tc * SP, axis=(-2, -1)).reshape(N_T, L, nv)
    f, fv = np.sum(w * tau), np.sum(w * dtau, axis=1)                  # f, f'_v
    f_i = np.einsum("k,knl->nl", w, tau_i)
    f_iv = np.einsum("k,knlv->nlv", w, tau_iv)
    if functional == SM:
        J = 1 - (f.real * f.real + f.imag * f.imag) / K ** 2
        G = -2 * (np.conj(f) * f_i).real / K ** 2
        Hv = -2 * (np.conj(fv)[None, None, :] * f_i[:, :, None] + np.conj(f) * f_iv).real / K ** 2
    elif functional == SS:
        J = 1 - np.sum(w * (tau.real * tau.real + tau.imag * tau.imag)) / K
        G = -2 * np.einsum("k,knl->nl", w, (np.conj(tau)[:, None, None] * tau_i).real) / K
        Hv = -2 * np.einsum("k,knlv->nlv", w, (np.conj(dtau.T)[:, None, None, :] * tau_i[..., None] + np.conj(tau)[:, None, None, None] * tau_iv).real) / K
    elif functional == RE:
        J = 1 - f.real / K
        G = -f_i.real / K
        Hv = -f_iv.real / K
    else:
        raise ValueError(f"functional {functional}")
    Hv = np.moveaxis(Hv, -1, 0).transpose(0, 2, 1).reshape(nv, L * N_T)          # [v][l][n]
    return dict(J=J, G=G.T.reshape(-1), tau=tau, Hv=Hv[0] if q["one"] else Hv, dtau=dtau)


# ---- the kernels' block recursion, in numpy -------------------------------------------------------------------------------
def _chain_series(step, Y, h, tol, max_terms=200):
    """sum_a y_a of a coupled stack: y_{a+1} = h / (a+1) step(y_a); stops when EVERY member has ||term|| <= tol ||sum|| (0 <= 0 counts)"""
    total, u = Y.copy(), Y
    for a in range(max_terms):
        u = step(u) * (h / (a + 1))
        total = total + u
        if np.all(orf._fro(u) <= tol * orf._fro(total)):
            return total
    raise ArithmeticError("open_hvp_reference.block_recursion: a series did not converge")


def block_recursion(pr, pulsevals, V, functional=0, theta=3.0, tol=1e-17, wrong=None, want_substeps=False):
    """Hv [nv, L*N_T] (or [L*N_T]) by the recursion of csrc/grape_lindblad_hvp.hip.h (complex128): stored rho_k(t_n) from a
    forward sweep, the tangent forward sweep (u, u') from the STORED states, chi'_k(T) = c'_k sigma_k, and per control the chains
    (c, c', p, p') under L^dagger, all carried over the m = ceil(beta dt / theta) sub-steps of an interval."""
    assert wrong is None or wrong in WRONG
    dtype = np.complex128
    q = _setup(pr, pulsevals, V, dtype)
    K, d, L, N_T, s, w, eps, Vs = q["K"], q["d"], q["L"], q["N_T"], q["s"], q["w"].copy(), q["eps"], q["V"]
    if wrong == "ignore_last_weight":
        w[-1] = 1.0
    sv = np.roll(s, -1, axis=0) if wrong == "shape_shift" else s        # the shape of control l + 1 applied to l (in B)
    nv = len(Vs)
    dts = np.diff(q["tl"])
    gens, store, dstore, msub = [], [], [], np.zeros((K, N_T), dtype=int)
    tau = np.empty(K, dtype=dtype)
    dtau = np.empty((nv, K), dtype=dtype)
    for k in range(K):
        Hc, cops = orf._per_k(q["Hc"], k, 3), orf._per_k(q["cops"], k, 3)
        copsd = orf._dag(cops)
        AdA = sum((copsd[j] @ cops[j] for j in range(len(cops))), np.zeros((d, d), dtype=dtype))
        D = -1j * Hc
        r0 = np.linalg.norm(q["H0"][k], 2)
        rl = [np.linalg.norm(Hc[l], 2) for l in range(L)]
        ra = sum(np.linalg.norm(A, 2) ** 2 for A in cops)
        gk = []
        rho = q["rho0"][k]
        st = [rho]
        for n in range(N_T):
            M = -1j * (q["H0"][k] + sum((s[l, n] * eps[l, n]) * Hc[l] for l in range(L))) - AdA / 2
            beta = 2 * (r0 + sum(abs(s[l, n] * eps[l, n]) * rl[l] for l in range(L))) + ra
            m = max(1, int(np.ceil(beta * dts[n] / theta)))
            msub[k, n] = m
            B = np.stack([sum((Vs[v, l, n] * sv[l, n]) * D[l] for l in range(L)) for v in range(nv)])
            gk.append(dict(M=M, Md=orf._dag(M), m=m, B=B, Bd=orf._dag(B), cops=cops, copsd=copsd, D=D, Dd=orf._dag(D)))
            lind = lambda X, g=gk[-1]: g["M"] @ X + X @ g["Md"] + sum((g["cops"][j] @ X @ g["copsd"][j] for j in range(len(g["cops"]))), 0 * X)  # noqa: E731
            Y = rho[None]
            for _ in range(m):
                Y = _chain_series(lind, Y, dts[n] / m, tol)
            rho = Y[0]
            st.append(rho)
        gens.append(gk)
        store.append(st)
        tau[k] = np.sum(np.conj(q["target"][k]) * rho)
        # tangent forward sweep, every direction: u_0 = the stored state, u'_0 = rho'(t_n)
        dk = np.zeros((nv, N_T + 1, d, d), dtype=dtype)
        for v in range(nv):
            for n in range(N_T):
                g = gk[n]

                def fwd(Y, g=g, v=v):
                    prim = g["M"] @ Y[1] + Y[1] @ g["Md"] + g["B"][v] @ Y[0] + Y[0] @ g["Bd"][v]
                    base = g["M"] @ Y[0] + Y[0] @ g["Md"]
                    for j in range(len(g["cops"])):
                        base = base + g["cops"][j] @ Y[0] @ g["copsd"][j]
                        if wrong != "no_dissipator_in_primed":
                            prim = prim + g["cops"][j] @ Y[1] @ g["copsd"][j]
                    return np.stack([base, prim])

                Y = np.stack([st[n], dk[v, n]])
                for _ in range(g["m"]):
                    Y = _chain_series(fwd, Y, dts[n] / g["m"], tol)
                dk[v, n + 1] = Y[1]
            dtau[v, k] = np.sum(np.conj(q["target"][k]) * dk[v, N_T])
        dstore.append(dk)
    f, fv = np.sum(w * tau), np.sum(w * dtau, axis=1)
    Hv = np.zeros((nv, L, N_T))
    for v in range(nv):
        for k in range(K):
            if functional == SM:
                c, cp = w[k] * f / K ** 2, w[k] * fv[v] / K ** 2
            elif functional == SS:
                c, cp = w[k] * tau[k] / K, w[k] * dtau[v, k] / K
            else:
                c, cp = w[k] / (2.0 * K), 0.0
            if wrong == "zero_chi_prime":
                cp = 0.0
            for l in range(L):
                chi, chip = c * q["target"][k], cp * q["target"][k] + 0j
                for n in range(N_T - 1, -1, -1):
                    g = gens[k][n]
                    Bd, B = (g["B"][v], g["Bd"][v]) if wrong == "swap_B_Bdag" else (g["Bd"][v], g["B"][v])
                    Dld, Dl, sh = g["Dd"][l], g["D"][l], s[l, n]

                    def bwd(Y, g=g, Bd=Bd, B=B, Dld=Dld, Dl=Dl, sh=sh):
                        cc, cq, pp, pq = Y

                        def adj(X, diss=True):
                            out = g["Md"] @ X + X @ g["M"]
                            if diss:
                                for j in range(len(g["cops"])):
                                    out = out + g["copsd"][j] @ X @ g["cops"][j]
                            return out

                        primed = wrong != "no_dissipator_in_primed"
                        o_c = adj(cc)
                        o_cq = Bd @ cc + cc @ B + adj(cq, primed)
                        o_p = sh * (Dld @ cc + cc @ Dl) + adj(pp)
                        o_pq = sh * (Dld @ cq + cq @ Dl) + adj(pq, primed)
                        if wrong != "drop_Bdag_p":
                            o_pq = o_pq + Bd @ pp + pp @ B
                        return np.stack([o_c, o_cq, o_p, o_pq])

                    Y = np.stack([chi, chip, np.zeros_like(chi), np.zeros_like(chi)])
                    for _ in range(g["m"]):
                        Y = _chain_series(bwd, Y, dts[n] / g["m"], tol)
                    chi, chip, P, Pp = Y
                    t = np.sum(np.conj(Pp) * store[k][n])
                    if wrong != "drop_rho_prime":
                        t = t + np.sum(np.conj(P) * dstore[k][v, n])
                    Hv[v, l, n] += -2.0 * t.real
    Hv = Hv.reshape(nv, L * N_T)
    out = Hv[0] if q["one"] else Hv
    return (out, msub) if want_substeps else out


# ---- inputs: the scheme of the open-system reference tests ----------------------------------------------------------------------
def directions(seed, nv, n):
    """nv deterministic O(1) directions of length n"""
    from grape_jl_amd import synth
    return 2.0 * synth.uniform01(synth.subseed(seed, 9100), nv * n).reshape(nv, n) - 1.0


_CACHE = {}


def reference_of(name, cases, nv=2):
    """(problem, V [nv, L*N_T], evaluate(...)) of a named case spec of open_time_reference.build_case: computed once, shared, never
    modified"""
    import open_time_reference as otr
    if name not in _CACHE:
        pr = otr.build_case(cases[name])
        V = directions(cases[name].get("seed", 0) + 17 * cases[name]["d"], cases[name].get("nv", nv), pr["pulsevals"].size)
        if cases[name].get("zero_interval") is not None:
            L = np.asarray(pr["Hc"]).shape[-3]
            V = V.reshape(len(V), L, -1).copy()
            V[0, :, cases[name]["zero_interval"]] = 0.0
            V = V.reshape(len(V), -1)
        _CACHE[name] = (pr, V, evaluate(pr, pr["pulsevals"], V, pr["functional"]))
    return _CACHE[name]
