"""Reference of grape_open_time_gradient (dJ/d dt_n on an open-system handle) in plain numpy, generic over
numpy.complex128 and numpy.clongdouble like open_reference.py, and the shared comparison of its tests.

The FORWARD sensitivity, not the kernel's adjoint form.  exp(L_n dt_n) commutes with L_n, so
    d rho(t_{n+1}) / d dt_n = sigma_n = L_n rho(t_{n+1}):
after interval n that matrix joins a stack which is propagated with rho through the remaining intervals, and
    dJ/d dt_n = -2 Re sum_k conj(c_k) <<sigma_k^tgt | sigma_n(T)>>,       chi_k(T) = c_k sigma_k^tgt (open_reference.functional_values)
(with ``boundary`` given: -2 Re sum_k <<chi_k | sigma_n(T)>>).  Sub-steps by open_reference.substeps (theta <= 1: the
reference's own rule), series until ||term||_F <= tol ||sum||_F for every member: tol = 1e-18 in double, 1e-24 in long double.
tests/test_open_time_reference.py proves it (central differences of J, scipy.linalg.expm, long double, the adjoint form) and
that the comparison below refuses subtly wrong references.
"""
import numpy as np

import open_helpers as oh
import open_reference as orf

SM, SS, RE = 0, 1, 2


def time_gradient(pr, pulsevals, functional=0, boundary=None, dtype=np.complex128, theta=1.0, tlist=None, shape=None, weights=None,
                  want_parts=False):
    """dJ/d dt_n [N_T] of the problem dicts of the open-system tests (open_reference.evaluate), in the real type of ``dtype``.
    ``want_parts``: dict(dJdt, tau [K], terms [K, N_T] = conj(c_k) <<sigma_k | sigma_n(T)>>, J) instead."""
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
    weights = pr.get("weights") if weights is None else weights
    rho0 = np.asarray(pr["rho0"], dtype=dtype)
    im = dtype(1j)
    rhoT = np.empty((K, d, d), dtype=dtype)
    sigT = np.empty((K, N_T, d, d), dtype=dtype)
    for k in range(K):
        Hc, cops = orf._per_k(Hc_all, k, 3), orf._per_k(cops_all, k, 3)
        copsd = orf._dag(cops)
        AdA = sum((copsd[j] @ cops[j] for j in range(len(cops))), np.zeros((d, d), dtype=dtype))
        Y = rho0[k][None]
        for n in range(N_T):
            H = H0[k] + sum((s[l, n] * eps[l, n]) * Hc[l] for l in range(L))
            M = -im * H - AdA / 2
            Md = orf._dag(M)

            def lind(X, M=M, Md=Md):
                out = M @ X + X @ Md
                for j in range(len(cops)):
                    out = out + cops[j] @ X @ copsd[j]
                return out

            dt = tl[n + 1] - tl[n]
            m = orf.substeps(M, cops, dt, theta)
            for _ in range(m):
                Y = orf._series(lind, Y, dt / m, tol, None)
            Y = np.concatenate([Y, lind(Y[:1])])          # sigma_n = L_n rho(t_{n+1}) joins the stack
        rhoT[k], sigT[k] = Y[0], Y[1:]
    if boundary is None:
        target = np.asarray(pr["target"], dtype=dtype)
        tau = np.sum(np.conj(target) * rhoT, axis=(-2, -1))
        J, c = orf.functional_values(tau, weights, functional)
        chi = np.asarray(c, dtype=dtype)[:, None, None] * target
    else:
        tau, J = None, None
        chi = np.asarray(boundary, dtype=dtype)
    terms = np.sum(np.conj(chi)[:, None] * sigT, axis=(-2, -1))     # <<chi_k | sigma_n(T)>>
    dJdt = -2 * np.sum(terms, axis=0).real
    return dict(dJdt=dJdt, tau=tau, terms=terms, J=J) if want_parts else dJdt


def tol_time(want):
    """the project's tol_G rule on the time gradient"""
    return 1e-10 * max(float(np.abs(want).max()), 1e-3)


def assert_order_one(want, tau):
    """the condition on the REFERENCE alone under which the bound of assert_time_gradient_agrees is relative, never its floor"""
    g_max = float(np.abs(np.asarray(want, dtype=float)).max())
    tau_min = float(np.abs(np.asarray(tau, dtype=complex)).min()) if tau is not None else None
    print(dict(dJdt_max=g_max, tau_min=tau_min))
    assert g_max >= 1e-3
    assert tau is None or tau_min >= 0.1


def assert_time_gradient_agrees(got, want, tau=None, label=""):
    """THE comparison of the time-gradient tests: ||got - want||_inf <= 1e-10 max(||want||_inf, 1e-3), after the condition on the
    reference (||want||_inf >= 1e-3; min_k |tau_k| >= 0.1 where the reference has a tau)."""
    want = np.asarray(want, dtype=float)
    got = np.asarray(got, dtype=float)
    assert_order_one(want, tau)
    assert got.shape == want.shape
    assert np.all(np.isfinite(got))
    dev = float(np.abs(got - want).max())
    print(label, dict(dev=dev, tol=tol_time(want), rel=dev / float(np.abs(want).max())))
    assert dev <= tol_time(want)
    return dev


# ---- inputs: the scheme of the open-system reference tests (synth.make_open_problem, open_helpers.order_one_states) ----------
def build_case(c):
    """Problem dict of a case spec: d, J, L, K, functional, and optionally N_T (3), weights, shape, nonuniform (dt in (0.5, 1.5)),
    cops_per_traj, hc_per_traj, hermitian, non_hermitian_states, non_hermitian_controls, long_step, dt, factor, seed."""
    from grape_jl_amd import synth
    d, J, L, K, N_T = c["d"], c["J"], c["L"], c["K"], c.get("N_T", 3)
    seed = c.get("seed", 2000 * d + 10 * J + L)
    pr = synth.make_open_problem(d, L, N_T, K, J, seed=seed, cops_per_traj=c.get("cops_per_traj", False),
                                 hermitian=c.get("hermitian", True))
    rng = np.random.default_rng(seed)
    dts = rng.uniform(0.5, 1.5, N_T) if c.get("nonuniform") else np.full(N_T, c.get("dt", 1.0))
    if c.get("long_step"):
        dts[1] *= c["long_step"]
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(dts)])
    pr["shape"] = rng.uniform(0.5, 1.0, (L, N_T)) if c.get("shape") else None
    pr["weights"] = np.array([0.5, 1.0, 1.5, 0.8])[:K] if c.get("weights") else None
    if c.get("hc_per_traj"):
        pr["Hc"] = np.stack([(1.0 + 0.3 * k) * pr["Hc"][::(-1 if k % 2 else 1)] for k in range(K)])
    if c.get("non_hermitian_controls"):
        z = synth.normal(synth.subseed(seed, 9000), 2 * L * d * d).reshape(2, L, d, d)
        pr["Hc"] = pr["Hc"] + 0.1 / np.sqrt(d) * (z[0] + 1j * z[1])
    pr["functional"] = c["functional"]
    return oh.order_one_states(pr, seed, factor=c.get("factor", 0.8), non_hermitian=c.get("non_hermitian_states", 0.0))


_CACHE = {}


def reference_of(name, cases):
    """(problem, time_gradient(..., want_parts=True)) of a named case: computed once, shared, never modified"""
    if name not in _CACHE:
        pr = build_case(cases[name])
        _CACHE[name] = (pr, time_gradient(pr, pr["pulsevals"], pr["functional"], want_parts=True))
    return _CACHE[name]
