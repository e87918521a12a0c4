"""Shared pieces of the open-system tests (tests/test_open_host.py, tests/test_gpu_open.py, tests/test_open_reference.py,
tests/test_gpu_open_reference.py): the comparison and the inputs of the reference tests, and the vectorised problem, built
HERE, with numpy.kron, independently of the product's ``liouvillian()`` -- that function is a thing under test."""
import numpy as np

TOL_J = 1e-12
TOL_TAU = 1e-12


def tol_G(G):
    return 1e-10 * max(np.abs(G).max(), 1e-3)


def open_figures(got, want):
    """worst deviation of every output ``want`` holds (J, tau, G, rhoT, tau_grads; got / want: dicts of those)"""
    fig = dict(tolG=tol_G(np.asarray(want["G"], dtype=float)))
    for key, name in (("J", "dJ"), ("tau", "dtau"), ("G", "dG"), ("rhoT", "drho"), ("tau_grads", "dtg")):
        if key in want:
            fig[name] = float(np.abs(np.asarray(got[key]) - np.asarray(want[key])).max())
    return fig


def assert_open_agrees(got, want, label=""):
    """THE comparison of the reference tests (tests/test_gpu_open_reference.py; tests/test_open_reference.py proves that it
    notices a subtly wrong side): the project's tolerances on every output."""
    fig = open_figures(got, want)
    print(label, fig)
    for key in ("J", "tau", "G", "rhoT", "tau_grads"):
        if key in want:
            assert np.shape(got[key]) == np.shape(want[key]), key
            assert np.all(np.isfinite(np.asarray(got[key], dtype=complex))), key
    assert fig.get("dJ", 0.0) <= TOL_J
    assert fig.get("dtau", 0.0) <= TOL_TAU
    assert fig.get("dG", 0.0) <= fig["tolG"]
    assert fig.get("drho", 0.0) <= 1e-12
    assert fig.get("dtg", 0.0) <= 1e-12
    return fig


def order_one_states(pr, seed, factor=0.8, non_hermitian=0.0):
    """Initial states and targets with O(1) signals, in place: rho_k(0) the projector on synth.unit_vectors, sigma_k the
    reference's rho_k(T) for the pulse factor * x scaled to unit Frobenius norm (so tau_k = O(1) and the gradient is far above
    the floor of tol_G).  non_hermitian > 0 adds a complex non-Hermitian part of that size to both."""
    import open_reference
    from grape_jl_amd import synth
    H0 = np.asarray(pr["H0"])
    K, d = H0.shape[0], H0.shape[1]
    v = synth.unit_vectors(synth.subseed(seed, 8000), K, d)
    pr["rho0"] = v[:, :, None] * v[:, None, :].conj()
    if non_hermitian:
        z = synth.normal(synth.subseed(seed, 8001), 4 * K * d * d).reshape(2, 2, K, d, d)
        pr["rho0"] = pr["rho0"] + non_hermitian / d * (z[0, 0] + 1j * z[0, 1])
    rhoT = open_reference.propagate(pr, factor * np.asarray(pr["pulsevals"]), gradient=False)["rhoT"]
    pr["target"] = rhoT / np.sqrt(np.sum(np.abs(rhoT) ** 2, axis=(-2, -1)))[:, None, None]
    if non_hermitian:
        pr["target"] = pr["target"] + non_hermitian / d * (z[1, 0] + 1j * z[1, 1])
    return pr


def assert_order_one(want):
    """the condition on the REFERENCE alone under which the floor of tol_G never engages"""
    tau_min, g_max = float(np.abs(want["tau"]).min()), float(np.abs(want["G"]).max())
    print(dict(tau_min=tau_min, G_max=g_max))
    assert tau_min >= 0.1
    assert g_max >= 1e-3


PIN_SPECS = {"d33": dict(d=33, J=3, K=2, seed=3303), "d48": dict(d=48, J=1, K=2, seed=4801), "d64": dict(d=64, J=8, K=1, seed=6408, factor=-0.8)}


def open_pin_problem(spec):
    """Inputs of a long-double pin (tests/golden/make_open_pins.py) from the synth seeds in ``spec``: L = 2, N_T = 3, weights,
    a shape and a non-uniform grid from the project's own generator, O(1) signals (d64: the target of the pulse -0.8 x, as
    eight collapse operators leave too small a gradient otherwise).  The targets come out of a double
    propagation, so they are rounded to multiples of 2^-30: the same doubles on every machine."""
    from grape_jl_amd import synth
    d, J, K, seed = spec["d"], spec["J"], spec["K"], spec["seed"]
    L, N_T = 2, 3
    pr = synth.make_open_problem(d, L, N_T, K, J, seed=seed)
    u = synth.uniform01(synth.subseed(seed, 8100), N_T + L * N_T)
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(0.5 + u[:N_T])])
    pr["shape"] = 0.5 + 0.5 * u[N_T:].reshape(L, N_T)
    pr["weights"] = np.array([1.5, 0.5])[:K]
    order_one_states(pr, seed, factor=spec.get("factor", 0.8))
    pr["target"] = np.round(pr["target"] * 2.0 ** 30) / 2.0 ** 30
    return pr


def load_open_pin(name):
    """(problem, {functional: dict(J, tau, G, tau_grads)}) of tests/golden/open_pin_<name>.json, rounded to double"""
    import json
    import os
    z = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"open_pin_{name}.json")))
    cf = lambda a: np.array(a, dtype=float)[..., 0] + 1j * np.array(a, dtype=float)[..., 1]   # noqa: E731
    want = {int(f): dict(J=float(v["J"]), tau=cf(v["tau"]), G=np.array(v["G"], dtype=float), tau_grads=cf(v["tau_grads"]))
            for f, v in z["functionals"].items()}
    return open_pin_problem(z["spec"]), want


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
