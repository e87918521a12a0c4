"""The inhomogeneous backward recursion on every sweep instantiation, and the balanced frame behind every entry point that
carries a state -- against tests/frame_reference.py (proved in tests/test_frame_reference.py).  Needs an MI355X.

Every case runs, on the reference's own propagation of one well-scaled twin:
  (a) the built-in running cost (Dpen, lambda_b): eval -> J, G, tau, sums()[4], time_gradient() = propagation + weight term;
  (b) a second handle without Dpen: forward, storage(0), backward_xi with g_b = <Psi|D|Psi>^2 -> G, storage(1), time_gradient()
      = the propagation part only (J_b is the caller's trapezoid sum on the handle's states);
  (c) backward_chi with an observable functional's chi -> G, storage(1)[:, -1], tau_grads;
  (d) backward_xi(..., chi=...) with both at once;
  (e) afterwards a plain eval: the built-in result (the custom sweeps leave nothing behind), final states, storage(1).
A balanced case hands the handle ``frame_reference.skewed(twin, e)`` and compares with the TWIN's reference, states and
propagators mapped back to the twin's frame; the twin itself runs through the same checks as the control.

Bars (frame_reference.assert_agrees): |dJ|, |dJ_b|, |dtau| <= 1e-12; states and propagators <= 1e-12 elementwise;
||dG||_inf <= 1e-10 max(||G||_inf, 1e-3), the same for dJdt and for tau_grads summed as G.  Every case asserts on the reference
alone min|tau_k| >= 0.1, ||G||_inf >= 1e-3, ||dJdt||_inf >= 1e-3, J_b >= 1e-2.  K <= 3, N_T <= 6, L <= 3 throughout.

Found by ``series-N320`` (a): gb_kernel (xi = -D Psi and g_b of the built-in running cost) handled 256 rows only, so above
N = 256 J_b, G and dJdt were wrong by O(1).
"""
import numpy as np
import pytest

import frame_reference as fr
import grape_jl_amd as g

pytestmark = pytest.mark.gpu

EXP, SER, GG, TY = g.PROP_EXP, g.PROP_SERIES, g.GRAD_GRADGEN, g.GRAD_TAYLOR


def T(N, kind="herm", L=2, K=2, N_T=4, per_traj=False, plain=False):
    return dict(N=N, kind=kind, L=L, K=K, N_T=N_T, per_traj=per_traj, plain=plain)


# ---- twins: one reference each, shared by every case that names it -------------------------------------------------------
TWINS = {
    # section 1: Hermitian, every padding and both edges of each
    "h16": T(16, L=3, K=3, N_T=6), "h17": T(17, K=3, N_T=5), "h32": T(32, per_traj=True), "h33": T(33, L=1, K=3),
    "h40": T(40, L=3), "h48": T(48, K=3), "h49": T(49, plain=True), "h64": T(64, L=3, N_T=5), "h65": T(65, L=1, K=2, N_T=3),
    "h100": T(100, L=2, K=2, N_T=3), "h128": T(128, L=1, K=2, N_T=3, plain=True), "h129": T(129, L=1, K=2, N_T=3),
    "h320": T(320, L=1, K=1, N_T=2),
    # sections 2 and 3: non-Hermitian twins of the skewed problems
    "g5": T(5, "general", K=2), "g16": T(16, "general", L=3, K=3, N_T=6), "d16": T(16, "general-drift", K=3, N_T=5),
    "g20": T(20, "general", K=3), "d33": T(33, "general-drift", L=1, K=3), "g40": T(40, "general", K=2, N_T=5),
    "g48": T(48, "general", K=2), "d57": T(57, "general-drift", L=3, K=2), "g64": T(64, "general", K=3, N_T=3),
    "g100": T(100, "general", L=1, K=2, N_T=3), "g130": T(130, "general", L=1, K=2, N_T=3),
}
_twins, _ctx = {}, {}


def seed_of(name):
    return 2000 + sum(map(ord, name))


def twin(name, functional):
    """(problems per mode, references per mode, exponents) of a twin under one functional: computed once and shared"""
    key = (name, functional)
    if key not in _twins:
        s = seed_of(name)
        if name not in _ctx:
            pr = fr.make_twin(seed=s, **TWINS[name])
            _ctx[name] = (pr, fr.propagate(pr, pr["pulsevals"]))
        pr, ctx = _ctx[name]
        # Dpen shared for odd N, one per trajectory for even N
        prs, want = fr.all_modes(pr, functional, s, per_traj_D=TWINS[name]["N"] % 2 == 0, ctx=ctx)
        _twins[key] = (prs, want, fr.skew_exponents(TWINS[name]["N"], s))
    return _twins[key]


def handle(p, functional, prop=EXP, method=GG, **kw):
    return g.GrapeHip(p["H0"], p["Hc"], p["tlist"], p["psi0"], p["target"], p["weights"], functional=functional,
                      shape=p["shape"], prop_method=prop, gradient_method=method, **kw)


def caller_side_cost(p, fw):
    """what the caller of grape_backward_xi computes on the handle's stored states: xi_k(t_n) and the trapezoid sum J_b"""
    K, M, _ = fw.shape
    xi = np.zeros_like(fw)
    gb = np.zeros((K, M))
    for k in range(K):
        for n in range(M):
            gb[k, n] = p["g_b"](fw[k, n], k, n)
            if n:
                xi[k, n] = p["xi"](fw[k, n], k, n)
    return xi, float(np.sum(gb * fr.trapezoid_weights(p["tlist"])[None, :]))


def run_modes(prs, want, functional, label, e=None, prop=EXP, method=GG, frame_getters=False):
    """(a)-(e) on two handles; ``prs`` in the caller's frame (skewed when ``e`` is given), ``want`` the twin's reference.
    Returns the measured deviations per mode."""
    x = prs["e"]["pulsevals"]
    dev = {}
    fr.assert_order_one(want["a"])
    fr.assert_order_one(want["b"])
    pa = prs["a"]
    with handle(pa, functional, prop, method, D=pa["D"], lambda_b=pa["lambda_b"]) as h:
        J, G, tau = h.eval(x)
        got = dict(J=J, G=G, tau=tau, Jb=h.sums()[4], dJdt=h.time_gradient())
    dev["a"] = fr.assert_agrees(got, want["a"], label + " (a)", e=e)
    pb = prs["b"]
    with handle(prs["e"], functional, prop, method) as h:
        got = dict(tau=h.forward(x), fw=h.storage(0))
        xi, got["Jb"] = caller_side_cost(pb, got["fw"])
        got.update(G=h.backward_xi(xi, pb["lambda_b"]), bw=h.storage(1), dJdt_prop=h.time_gradient())
        dev["b"] = fr.assert_agrees(got, want["b"], label + " (b)", e=e)
        h.forward(x)
        got = dict(G=h.backward_chi(prs["c"]["chi"]), bwT=h.storage(1)[:, -1], tau_grads=h.tau_grads())
        dev["c"] = fr.assert_agrees(got, want["c"], label + " (c)", e=e)
        h.forward(x)
        got = dict(G=h.backward_xi(xi, pb["lambda_b"], chi=prs["d"]["chi"]), bw=h.storage(1), dJdt_prop=h.time_gradient())
        dev["d"] = fr.assert_agrees(got, want["d"], label + " (d)", e=e)
        J, G, tau, psiT = h.eval(x, want_psiT=True)
        got = dict(J=J, G=G, tau=tau, psiT=psiT, dJdt=h.time_gradient(), bw=h.storage(1), tau_grads=h.tau_grads())
        if frame_getters:
            k, n = prs["e"]["K"] - 1, 1
            assert np.array_equal(h.final_states(), psiT)
            if prop == EXP:
                got.update(U=h.propagator(k, n), Ukn=(k, n))
        dev["e"] = fr.assert_agrees(got, want["e"], label + " (e)", e=e)
    return dev


# ---- 1. sweep instantiations x inhomogeneity -----------------------------------------------------------------------------
# name: (twin, functional, prop_method, gradient_method); the functionals are spread over the sizes, one GRAPE_GRAD_TAYLOR case at
# each of NP = 32, 48, 64
SWEEPS = {
    "exp-N16": ("h16", 0, EXP, GG), "exp-N17": ("h17", 1, EXP, GG), "exp-N32-taylor": ("h32", 2, EXP, TY),
    "exp-N33": ("h33", 0, EXP, GG), "exp-N48-taylor": ("h48", 1, EXP, TY), "exp-N49": ("h49", 2, EXP, GG),
    "exp-N64-taylor": ("h64", 0, EXP, TY), "exp-N65": ("h65", 1, EXP, GG), "exp-N128": ("h128", 2, EXP, GG),
    "exp-N129": ("h129", 0, EXP, GG),
    "series-N16": ("h16", 1, SER, GG), "series-N17": ("h17", 2, SER, GG), "series-N32": ("h32", 0, SER, GG),
    "series-N40-repadded": ("h40", 1, SER, GG), "series-N64": ("h64", 2, SER, GG), "series-N100-chebyshev": ("h100", 0, SER, GG),
    "series-N320": ("h320", 1, SER, GG),
}


@pytest.mark.parametrize("name", list(SWEEPS))
def test_inhomogeneous_recursion_on_every_sweep(name):
    tw, f, prop, method = SWEEPS[name]
    prs, want, _ = twin(tw, f)
    run_modes(prs, want, f, name, prop=prop, method=method)


# ---- 2. balanced frame, every route --------------------------------------------------------------------------------------
# name: (twin, functional, prop_method, gradient_method, environment, remove the GRAPE_DERIV3 pin of the session)
FRAMES = {
    "N16-general-scan0": ("g16", 0, EXP, GG, {"GRAPE_SCAN16": "0"}, False),
    "N16-general-drift-scan1": ("d16", 1, EXP, GG, {"GRAPE_SCAN16": "1"}, False),
    "N20-general": ("g20", 2, EXP, GG, {}, False), "N20-general-taylor": ("g20", 0, EXP, TY, {}, False),
    "N33-general-drift": ("d33", 1, EXP, GG, {}, False),
    "N48-general": ("g48", 2, EXP, GG, {}, False), "N48-general-taylor": ("g48", 0, EXP, TY, {}, False),
    "N48-general-default-derivative": ("g48", 1, EXP, GG, {}, True),
    "N57-general-drift": ("d57", 2, EXP, GG, {}, False),
    "N64-general": ("g64", 0, EXP, GG, {}, False), "N64-general-taylor": ("g64", 1, EXP, TY, {}, False),
    "N64-general-default-derivative": ("g64", 2, EXP, GG, {}, True),
    "N100-general-blocked": ("g100", 0, EXP, GG, {}, False), "N130-general-blocked": ("g130", 1, EXP, GG, {}, False),
    "series-N20-general": ("g20", 1, SER, GG, {}, False), "series-N40-general": ("g40", 2, SER, GG, {}, False),
    "series-N64-general": ("g64", 1, SER, GG, {}, False), "series-N100-general-substeps": ("g100", 2, SER, GG, {}, False),
}


def skewed_modes(prs, e):
    return {m: fr.skewed(p, e) for m, p in prs.items()}


@pytest.mark.parametrize("name", list(FRAMES))
def test_balanced_frame_on_every_route(monkeypatch, name):
    tw, f, prop, method, env, unpin = FRAMES[name]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    if unpin:   # the derivative route small problems get by default (tests/test_gpu_scan.py removes the pin the same way)
        monkeypatch.delenv("GRAPE_DERIV3", raising=False)
    prs, want, e = twin(tw, f)
    control = run_modes(prs, want, f, name + " twin", prop=prop, method=method, frame_getters=True)
    skew = run_modes(skewed_modes(prs, e), want, f, name + " skewed", e=e, prop=prop, method=method, frame_getters=True)
    for m in skew:
        print(name, m, "skewed / twin:", {q: "%.1e / %.1e" % (skew[m][q], control[m][q]) for q in skew[m]})


# one per size class (padding 16, 32, 48, 64, 128, 256) and one on the matrix-free propagator
NONTRIVIAL = ["N16-general-scan0", "N20-general", "N33-general-drift", "N64-general", "N100-general-blocked",
              "N130-general-blocked", "series-N40-general"]


@pytest.mark.parametrize("name", NONTRIVIAL)
def test_the_frame_is_not_trivial(monkeypatch, name):
    """the same handle under GRAPE_BALANCE=0 (read at create) returns a G that is not bit-identical to the default's: the
    balancing of the skewed problem is not the identity, so the cases above do test the frame code"""
    tw, f, prop, method, env, _ = FRAMES[name]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    prs, want, e = twin(tw, f)
    p = fr.skewed(prs["e"], e)
    with handle(p, f, prop, method) as h:
        _, G1, _ = h.eval(p["pulsevals"])
    monkeypatch.setenv("GRAPE_BALANCE", "0")
    with handle(p, f, prop, method) as h:
        _, G0, _ = h.eval(p["pulsevals"])
    print(name, dict(balanced=float(np.abs(G1 - want["e"]["G"]).max()), unbalanced=float(np.abs(G0 - want["e"]["G"]).max()),
                     tol=fr.tol_G(want["e"]["G"])))
    assert not np.array_equal(G0, G1)


# ---- 3. the frame behind the other entry points --------------------------------------------------------------------------

@pytest.mark.parametrize("tw,f", [("g5", 0), ("g16", 1)])
def test_batched_kernels_in_the_callers_frame(monkeypatch, tw, f):
    monkeypatch.setenv("GRAPE_BATCH", "1")
    prs, want, e = twin(tw, f)
    p = fr.skewed(prs["e"], e)
    x = p["pulsevals"]
    X = np.stack([x, 0.9 * x, 1.1 * x])
    wants = [want["e"]] + [fr.evaluate(prs["e"], xx, f) for xx in X[1:]]
    with handle(p, f) as h:
        J, G, tau = h.eval_batch(X)
        assert h.batch_info()["route"] == 1, h.batch_info()
    for i, w in enumerate(wants):
        fr.assert_order_one(w, running_cost=False)
        fr.assert_agrees(dict(J=J[i], G=G[i], tau=tau[i]), w, f"{tw} batch set {i}", e=e)


@pytest.mark.parametrize("tw,f", [("g20", 1), ("g64", 2)])
def test_composite_handle_in_the_callers_frame(tw, f):
    """devices = [0, 0]: multi_create forces ONE similarity on both shards; with the built-in running cost"""
    prs, want, e = twin(tw, f)
    pa = fr.skewed(prs["a"], e)
    x = pa["pulsevals"]
    chi_twin = prs["c"]["chi"]
    want_chi = fr.evaluate(dict(prs["a"], chi=chi_twin), x, f)
    fr.assert_order_one(want["a"])
    with handle(pa, f, D=pa["D"], lambda_b=pa["lambda_b"], devices=[0, 0]) as h:
        J, G, tau, psiT = h.eval(x, want_psiT=True)
        got = dict(J=J, G=G, tau=tau, psiT=psiT, Jb=h.sums()[4], fw=h.storage(0), dJdt=h.time_gradient(), tau_grads=h.tau_grads())
        assert np.array_equal(h.final_states(), psiT)
        fr.assert_agrees(got, want["a"], tw + " composite", e=e)
        h.forward(x)
        got = dict(G=h.backward_chi(fr.skewed(dict(prs["a"], chi=chi_twin), e)["chi"]), bwT=h.storage(1)[:, -1])
        fr.assert_agrees(got, want_chi, tw + " composite chi", e=e)


def test_split_phase_shards_balance_on_their_own():
    """K_total = 3 in slices of 1 and 2 trajectories at N = 33: each shard balances from its own generators"""
    f = 0
    prs, want, e = twin("d33", f)
    pa = fr.skewed(prs["a"], e)
    x, K = pa["pulsevals"], 3
    w = want["a"]
    fr.assert_order_one(w)
    shards = []
    for lo, hi in ((0, 1), (1, 3)):
        sl = slice(lo, hi)
        h = g.GrapeHip(pa["H0"][sl], pa["Hc"], pa["tlist"], pa["psi0"][sl], pa["target"][sl], pa["weights"][sl], functional=f,
                       shape=pa["shape"], K_total=K, D=pa["D"], lambda_b=pa["lambda_b"])
        tau = h.forward(x)
        shards.append((h, sl, tau, h.sums(), h.storage(0)))
    ftot = sum(complex(s[0], s[1]) for _, _, _, s, _ in shards)
    Jb = sum(s[4] for _, _, _, s, _ in shards)
    G, dJdt = np.zeros_like(w["G"]), np.zeros_like(w["dJdt"])
    for h, sl, tau, _, fw in shards:
        G += h.backward(ftot)
        dJdt += h.time_gradient()
        h.close()
        fr.assert_agrees(dict(tau=tau, fw=fw), dict(tau=w["tau"][sl], fw=w["fw"][sl]), f"shard {sl.start}:{sl.stop}", e=e)
    fr.assert_agrees(dict(J=1.0 - abs(ftot) ** 2 / K ** 2 + pa["lambda_b"] * Jb, Jb=Jb, G=G, dJdt=dJdt), w, "shards summed", e=e)


def test_set_tlist_keeps_the_frame():
    f = 1
    prs, want, e = twin("g40", f)
    pa = fr.skewed(prs["a"], e)
    x = pa["pulsevals"]
    fr.assert_order_one(want["a"])
    first = np.linspace(0.0, 0.6 * pa["tlist"][-1], len(pa["tlist"]))
    with handle(dict(pa, tlist=first), f, D=pa["D"], lambda_b=pa["lambda_b"]) as h:
        h.eval(x)
        h.set_tlist(pa["tlist"])
        J, G, tau, psiT = h.eval(x, want_psiT=True)
        got = dict(J=J, G=G, tau=tau, psiT=psiT, Jb=h.sums()[4], fw=h.storage(0), dJdt=h.time_gradient(), bw=h.storage(1))
    fr.assert_agrees(got, want["a"], "after set_tlist", e=e)
