"""Reference of the decisions behind the four-product route (numpy, float64 + eigvalsh), restated from the formulas above
t16_plan_kernel (grape.jl_amd/csrc/grape_kernels.hip.h) and DESIGN.md section 4.1 -- and the inputs that put cells at the
edges of its certified range.  Used by tests/test_t16_route_reference.py (CPU) and tests/test_gpu_t16_edges.py (GPU).

Per cell of a generator class (kc, n), with e = (1, eps_1 S_1, .., eps_L S_L), H = H0 + sum_l e_l C_l, dt = dts[n]:

  plan         r = 2 |dt| sqrt(e^T G e / N) kappa,  kappa = sum_a |e_a| f_a kappa_a / sum_a |e_a| f_a,  f_a = ||O_a||_F,
               kappa_a = ||O_a||_S8 / (3.5^(1/8) 2 f_a / sqrt(N));  s = 0 if r <= 1.15, else the smallest s <= 3 with
               r / 2^s <= 1.11; none: the cell is out of range (s = 0).  More than a quarter out of range: the route is not tried.
  certificate  (p8 + 2^-30 S8) dt^8 (1 + 1e-6) <= (theta 2^s)^8 and p6 >= 0, p8, p6, S8 from the trace tables
  the cell     m8 (1 + 1e-9) <= theta^8 and m6 >= 0 on the eigenvalues of H dt / 2^s, or ||(A / 2^s)^2||_1 (1 + 1e-9) <= theta^2

delta = m8 dt^8 / (theta 2^s)^8 - 1 measures the distance from the edge.  A cell is UNDECIDABLE when the device's own
rounding could decide either way: delta in [-2e-6, -5e-7] (certificate), |delta| < 1e-8 (cell), a plan threshold within 1e-6
relative, the 1-norm test within 10 % when it is the one that decides.  Every input of the GPU tests has no such cell."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from grape_jl_amd import synth  # noqa: E402
from test_cert_table import evaluate, trace_tables  # noqa: E402

THETA = 1.36
PLAN_R, PLAN_RS, PLAN_SMAX = 1.15, 1.11, 3
CERT_LMAX = 4
CERTIFIED, PASSED, HANDED, UNDECIDABLE = "certified", "passed by the cell", "handed over", "undecidable"


# ---------------------------------------------------------------- decisions
def classes(pr):
    """generator class of every trajectory (identical drift and controls share one), in order of first appearance"""
    K = pr["H0"].shape[0]
    per = np.asarray(pr["Hc"]).ndim == 4
    cls, reps = [], []
    for k in range(K):
        for c, r in enumerate(reps):
            if np.array_equal(pr["H0"][k], pr["H0"][r]) and (not per or np.array_equal(pr["Hc"][k], pr["Hc"][r])):
                cls.append(c)
                break
        else:
            cls.append(len(reps))
            reps.append(k)
    return cls, reps


def operators(pr, k):
    Hc = pr["Hc"][k] if np.asarray(pr["Hc"]).ndim == 4 else pr["Hc"]
    return [pr["H0"][k]] + [Hc[l] for l in range(Hc.shape[0])]


def amplitudes(pr, n):
    N_T = len(pr["tlist"]) - 1
    L = pr["pulsevals"].size // N_T
    e = pr["pulsevals"].reshape(L, N_T)[:, n].copy()
    if pr.get("shape") is not None:
        e = e * np.asarray(pr["shape"]).reshape(L, N_T)[:, n]
    return e


def shape_factor(O):
    N = O.shape[0]
    f2 = np.sum(np.abs(O) ** 2)
    if not f2 > 0.0:
        return 1.0
    O4 = np.linalg.matrix_power(O, 4)
    s8 = np.sum(np.abs(O4) ** 2) ** 0.125                   # ||O||_S8^8 = ||O^4||_F^2 for a Hermitian O
    return s8 / (3.5 ** 0.125 * 2.0 * np.sqrt(f2 / N))


def plan_estimate(ops, e, dt):
    N = ops[0].shape[0]
    ee = np.concatenate([[1.0], e])
    G = np.array([[np.sum(a.conj() * b).real for b in ops] for a in ops])
    kap = np.array([shape_factor(O) for O in ops])
    w = np.abs(ee) * np.sqrt(np.maximum(np.diag(G), 0.0))
    return 2.0 * abs(dt) * np.sqrt(max(ee @ G @ ee, 0.0) / N) * (np.sum(w * kap) / np.sum(w) if np.sum(w) > 0 else 1.0)


def plan_squarings(r, sq_on=True):
    """(s, out of range, within 1e-6 of a threshold)"""
    near = abs(r / PLAN_R - 1.0) < 1e-6
    if r <= PLAN_R:
        return 0, False, near
    if not sq_on:
        return 0, True, near
    rs, s = r, 0
    while s < PLAN_SMAX and not rs <= PLAN_RS:
        rs *= 0.5
        s += 1
        near = near or abs(rs / PLAN_RS - 1.0) < 1e-6
    out = not rs <= PLAN_RS
    return (0 if out else s), out, near


def decide(pr, cert=True, sq_on=True):
    """the route of every cell: dict(kind [KC][N_T], sq, delta, r, out, skipped, counts, tables)"""
    cls, reps = classes(pr)
    KC, N_T = len(reps), len(pr["tlist"]) - 1
    dts = np.diff(pr["tlist"])
    L = pr["pulsevals"].size // N_T
    kind = [[None] * N_T for _ in range(KC)]
    sq = np.zeros((KC, N_T), int)
    delta, rr = np.zeros((KC, N_T)), np.zeros((KC, N_T))
    nout, tables = 0, []
    for kc, k in enumerate(reps):
        ops = operators(pr, k)
        tab = trace_tables(ops) if cert and 1 <= L <= CERT_LMAX else None
        tables.append(tab)
        for n in range(N_T):
            e, dt = amplitudes(pr, n), dts[n]
            H = ops[0] + sum(e[l] * ops[1 + l] for l in range(L))
            lam = np.linalg.eigvalsh(H)
            r = plan_estimate(ops, e, dt)
            s, out, near = plan_squarings(r, sq_on)
            nout += out
            sq[kc, n], rr[kc, n] = s, r
            edge8 = (THETA * 2.0 ** s) ** 8
            m8 = np.sum(lam ** 8)
            d = m8 * dt ** 8 / edge8 - 1.0
            delta[kc, n] = d
            und = near
            certified = False
            if tab is not None:
                t8, t6, ex8, ex6 = tab
                p8, S8 = evaluate(t8, ex8, e)
                p6, _ = evaluate(t6, ex6, e)
                certified = (p8 + 2.0 ** -30 * S8) * dt ** 8 * (1.0 + 1e-6) <= edge8 and p6 >= 0.0
                und = und or -2e-6 <= d <= -5e-7
            schatten = m8 * dt ** 8 * (1.0 + 1e-9) <= edge8
            und = und or abs(d) < 1e-8
            A2 = (H @ H) * (dt / 2.0 ** s) ** 2
            n2 = (np.abs(A2.real) + np.abs(A2.imag)).sum(axis=0).max() / THETA ** 2
            one_norm = n2 * (1.0 + 1e-9) <= 1.0
            if not schatten and 0.9 <= n2 <= 1.1:
                und = True
            kind[kc][n] = UNDECIDABLE if und else CERTIFIED if certified else PASSED if (schatten or one_norm) else HANDED
    ncell = KC * N_T
    skipped = 4 * nout > ncell
    flat = [x for row in kind for x in row]
    counts = dict(certified=0 if skipped else flat.count(CERTIFIED),
                  t16_cells=0 if skipped else flat.count(CERTIFIED) + flat.count(PASSED),
                  handed_over=ncell if skipped else flat.count(HANDED), undecidable=flat.count(UNDECIDABLE), out=nout, ncell=ncell,
                  squarings_kept=0 if skipped else int(sum(sq[kc, n] for kc in range(KC) for n in range(N_T) if kind[kc][n] in (CERTIFIED, PASSED))))
    return dict(kind=kind, sq=sq, delta=delta, r=rr, skipped=skipped, counts=counts, cls=cls, reps=reps, tables=tables)


def econ_batches(dec):
    """what deriv_econ_kernel gives every batch of 16 steps of every trajectory: the radius of the economized series (1.36 when
    all cells kept by the four-product route have s = 0, 2.72 with s <= 1) or 0 (Taylor series)"""
    N_T = len(dec["kind"][0])
    out = []
    for k, kc in enumerate(dec["cls"]):
        row = []
        for n0 in range(0, N_T, 16):
            cells = range(n0, min(n0 + 16, N_T))
            ok = not dec["skipped"] and all(dec["kind"][kc][n] in (CERTIFIED, PASSED) and dec["sq"][kc, n] <= 1 for n in cells)
            row.append(0.0 if not ok else THETA * 2.0 ** max(dec["sq"][kc, n] for n in cells))
        out.append(row)
    return out


# ---------------------------------------------------------------- values
def propagators(pr):
    """U[k][n] = V exp(-i lam dt) V^dagger, with the eigendecompositions for the gradient"""
    K, N_T = pr["H0"].shape[0], len(pr["tlist"]) - 1
    dts = np.diff(pr["tlist"])
    N = pr["H0"].shape[1]
    U = np.empty((K, N_T, N, N), complex)
    eig = {}
    for k in range(K):
        ops = operators(pr, k)
        for n in range(N_T):
            e = amplitudes(pr, n)
            lam, V = np.linalg.eigh(ops[0] + sum(e[l] * ops[1 + l] for l in range(len(e))))
            U[k, n] = (V * np.exp(-1j * lam * dts[n])) @ V.conj().T
            eig[(k, n)] = (lam, V)
    return U, eig


def evaluate_dk(pr, functional=0):
    """J, tau, G, Psi(T), tau_grads [K][L][N_T] and U by eigendecomposition + Daleckii-Krein divided differences in double
    (the formulas of tests/golden/make_mpmath_pin64.py); the divided differences are taken as
    exp((x_i + x_j) / 2) sinc-form, which does not cancel for close eigenvalues"""
    K, N_T = pr["H0"].shape[0], len(pr["tlist"]) - 1
    N = pr["H0"].shape[1]
    dts = np.diff(pr["tlist"])
    L = pr["pulsevals"].size // N_T
    w = np.asarray(pr["weights"], float)
    U, eig = propagators(pr)
    st = np.empty((K, N_T + 1, N), complex)
    st[:, 0] = pr["psi0"]
    for k in range(K):
        for n in range(N_T):
            st[k, n + 1] = U[k, n] @ st[k, n]
    tgt = pr["target"]
    tau = np.array([np.vdot(tgt[k], st[k, N_T]) for k in range(K)])
    f = np.sum(w * tau)
    if functional == 0:
        J, chi = 1.0 - abs(f) ** 2 / K ** 2, [(w[k] * f / K ** 2) * tgt[k] for k in range(K)]
    elif functional == 1:
        J, chi = 1.0 - np.sum(w * np.abs(tau) ** 2) / K, [(w[k] * tau[k] / K) * tgt[k] for k in range(K)]
    else:
        J, chi = 1.0 - f.real / K, [(w[k] / (2.0 * K)) * tgt[k] for k in range(K)]
    shape = None if pr.get("shape") is None else np.asarray(pr["shape"]).reshape(L, N_T)
    tg = np.zeros((K, L, N_T), complex)
    for k in range(K):
        rho = np.linalg.norm(chi[k])
        chik = chi[k] / rho
        ops = operators(pr, k)
        for n in range(N_T - 1, -1, -1):
            lam, V = eig[(k, n)]
            dt = dts[n]
            x = dt * lam
            half = 0.5 * (x[:, None] - x[None, :])
            gam = np.exp(0.5j * (x[:, None] + x[None, :])) * np.sinc(half / np.pi)       # (e^{i x_i} - e^{i x_j}) / (i (x_i - x_j))
            c = V.conj().T @ chik
            for l in range(L):
                mu = ops[1 + l] * (1.0 if shape is None else shape[l, n])
                Et = V.conj().T @ (1j * dt * mu.conj().T) @ V
                tg[k, l, n] = rho * np.vdot(V @ ((Et * gam) @ c), st[k, n])
            chik = V @ (np.exp(1j * x) * c)
    G = -2.0 * tg.sum(axis=0).real.reshape(-1)
    return dict(J=J, tau=tau, G=G, psiT=st[:, N_T].copy(), tau_grads=tg, U=U)


# ---------------------------------------------------------------- inputs at the edges
N, K, N_T = 64, 3, 24
KSTAR = 0
TRAJ_SHIFT = (0.0, -0.03, 0.025)         # the other trajectories move the outlier eigenvalue by a few percent
# (step, planned squarings of the edge, delta): the first derivative batch of a trajectory is n = 0 .. 15, the ragged last one
# n = 16 .. 23.  The s = 2 edges sit in the last batch only, so the first batch of the trajectory 3 % inside holds nothing but
# certified cells with s <= 1 -- the economized series runs there, at both of its radii.
EDGE_STEPS = ((1, 0, -1e-3), (3, 0, -1e-5), (5, 0, -1e-7), (7, 0, 1e-7), (9, 0, 1e-3),
              (11, 1, -1e-3), (13, 1, -1e-5), (14, 1, -1e-7), (17, 1, 1e-7), (18, 1, 1e-3),
              (20, 2, -1e-5), (22, 2, 1e-3))
EXPECTED = {-1e-3: CERTIFIED, -1e-5: CERTIFIED, -1e-7: PASSED, 1e-7: HANDED, 1e-3: HANDED}
INTERIOR_DT = (1.0, 0.7, 1.2, 0.9)


def projector():
    u = synth.unit_vectors(13, 1, N)[0]
    P = np.outer(u, u.conj())
    return 0.5 * (P + P.conj().T)        # Hermitian to the last bit (the handle takes nothing else for a Hermitian generator)


def m8_of(pr, k, n):
    ops = operators(pr, k)
    e = amplitudes(pr, n)
    lam = np.linalg.eigvalsh(ops[0] + sum(e[l] * ops[1 + l] for l in range(len(e))))
    return np.sum(lam ** 8), lam


def edge_dt(pr, k, n, s, delta):
    return 2.0 ** s * THETA * (1.0 + delta) ** 0.125 / m8_of(pr, k, n)[0] ** 0.125


def edge_problem(variant="base"):
    """variant: base | pertraj (control operators per trajectory, expm_t16p_asm) | shape (S = 2 at two steps) | negative (eps < 0)"""
    P = projector()
    C2 = 0.3 * synth.gue(11, N)
    D = 0.3 * synth.gue(7, N)
    sign = -1.0 if variant == "negative" else 1.0
    if variant == "pertraj":
        H0 = np.stack([D.copy() for _ in range(K)])
        Hc = np.stack([np.stack([(1.0 + a) * P, C2]) for a in TRAJ_SHIFT])
    else:
        H0 = np.stack([D + sign * a * P for a in TRAJ_SHIFT])
        Hc = np.stack([P, C2])
    pulse = np.concatenate([np.full(N_T, sign * 1.0), np.full(N_T, sign * 0.1)])
    pr = dict(N=N, L=2, N_T=N_T, K=K, H0=H0, Hc=Hc, psi0=synth.unit_vectors(21, K, N), target=synth.unit_vectors(22, K, N),
              pulsevals=pulse, weights=np.ones(K), shape=None, tlist=np.arange(N_T + 1.0))
    dts = np.array([INTERIOR_DT[n % 4] for n in range(N_T)])
    steps = list(EDGE_STEPS)
    if variant == "s01":       # without the s = 2 edges: with GRAPE_EXPM_SQ=0 the 15 cells with s >= 1 stay below the quarter rule
        steps = [x for x in steps if x[1] < 2]
    if variant == "shape":
        shape = np.ones((2, N_T))
        shape[0, 2] = shape[0, 19] = 2.0              # two interior steps: the shape alone doubles the control there
        pr["shape"] = shape
        steps += [(2, 0, -1e-5), (19, 0, 1e-3)]
    for n, s, delta in steps:
        dts[n] = edge_dt(pr, KSTAR, n, s, delta)
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(dts)])
    # (the cumulative sum rounds: the device and the reference both take dt_n = tlist[n + 1] - tlist[n], which moves delta by a
    # few 1e-16 * 8 * t / dt -- checked in test_t16_route_reference.py against the guard bands)
    pr["edge_steps"] = steps
    return pr


def quarter_problem():
    """7 of 24 steps beyond 2^3 x range by a pulse value of 4 pi (as in test_a_cell_beyond_the_bound...), the rest certifiable"""
    pr = synth.make_problem(N, 2, N_T, K, seed=3)
    pr["shape"] = None
    for n in (0, 3, 6, 10, 15, 16, 23):
        pr["pulsevals"][n] = 4.0 * np.pi
    return pr


def stale_problem():
    """K = 2, N_T = 24 on the generator of the edge inputs; cells X = (0, 4) and Y = (0, 20) sit 2e-3 inside the s = 0 edge at
    pulse value 1.  Pulses A raise the first control at X by 1 % (X beyond, Y inside), pulses B at Y; grid2 shortens step X by 2 %."""
    pr = edge_problem("base")
    X, Y = 4, 20
    pr.update(K=2, H0=pr["H0"][:2], psi0=pr["psi0"][:2], target=pr["target"][:2], weights=np.ones(2))
    dts = np.array([INTERIOR_DT[n % 4] for n in range(N_T)])
    for n in (X, Y):
        dts[n] = edge_dt(pr, KSTAR, n, 0, -2e-3 * 8)
    pr["tlist"] = np.concatenate([[0.0], np.cumsum(dts)])
    A, B = pr["pulsevals"].copy(), pr["pulsevals"].copy()
    A[X] = 1.01
    B[Y] = 1.01
    dts2 = dts.copy()
    dts2[X] *= 0.98
    return pr, A, B, np.concatenate([[0.0], np.cumsum(dts2)]), X, Y


def with_pulses(pr, x, tlist=None):
    out = dict(pr)
    out["pulsevals"] = np.asarray(x, float).copy()
    if tlist is not None:
        out["tlist"] = np.asarray(tlist, float).copy()
    return out


# ---------------------------------------------------------------- tables beyond three classes
def table_problem(case):
    """the cases a .. e of the table build (classes per pass of 64 MB: 29 at L = 2, 14 at L = 3, 8 at L = 4)"""
    Nn, L, Kk = {"a": (64, 2, 31), "b": (64, 3, 15), "c": (64, 4, 9), "d": (50, 2, 3), "e": (64, 2, 4)}[case]
    pr = synth.make_problem(Nn, L, 2, Kk, seed=700 + ord(case))
    pr["shape"] = None
    if case == "e":                                    # two distinct drifts: trajectories 0, 2 and 1, 3 share theirs
        pr["H0"][2], pr["H0"][3] = pr["H0"][0], pr["H0"][1]
    return pr
