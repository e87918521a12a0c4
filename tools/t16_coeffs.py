"""Coefficients of the four-product degree-16 polynomial evaluation used by the Hermitian exponential for spectral radii up
to T16_THETA (grape_t18.hip.h: expm_t16_*).

Evaluation scheme (Sastre 2018, "Efficient evaluation of matrix polynomials", the m = 15+ formulas; restated here from the
published algorithm, the coefficients are recomputed from scratch -- a multi-start least-squares search for the Taylor
solution, kept below as START, then Newton in 80 digits):

    A2  = A A
    y0  = A2 (c1 A2 + c2 A)
    y1  = (y0 + c3 A2 + c4 A)(y0 + c5 A2) + c6 y0 + c7 A2
    p   = (y1 + c8 A2 + c9 A)(y1 + c10 y0 + c11 A) + c12 y1 + c13 y0 + c14 A2 + c15 A + c16 I      (degree 16, four products)

16 parameters for the 17 coefficients of a degree-16 polynomial: b_0..b_15 can be prescribed, b_16 = c1^4 follows.
Two targets:

  * ``taylor``: b_k = 1/k!, k <= 15 (b_16 comes out as 0.5457/16!)
  * ``cheb(beta)``: on the segment x = -i lam, |lam| <= beta, the polynomial q15(x) - b_16 r(x) + b_16 x^16 where q15 is the
    degree-15 Chebyshev truncation of exp and r(x) = x^16 - beta^16 2^-15 T_16(lam/beta) is the part of x^16 that polynomials
    of degree <= 14 can absorb.  The error on the segment is then |2 J_16(beta) - b_16 beta^16 / 2^15| + 2 J_17(beta) + ...
    = about 0.45 * 2 J_16(beta): 1e-16 at beta = 1.36.

Run:  python3 tools/t16_coeffs.py [beta]     prints C initialisers and the achieved error on the segment.

Mode ``q`` -- the set T16Q_* whose second product is a Hermitian square.  With c2 = 0 the second product is y0 = c1 A2 A2, the
square of a Hermitian matrix (half the tiles, like A A).  Then y1 has no x^7 term and p no x^15 term: b_15 = 0 is structural,
15 parameters (c1, c3..c16) are left for b_0..b_14, and b_16 = c1^4 follows as before.  Target on the segment: the degree-14
Chebyshev truncation q14 with the absorbable part of b_16 x^16 taken out as above; the T_15 term is not represented, so the
error is 2 J_15(beta) + |2 J_16(beta) - b_16 beta^16 / 2^15| + ... : 2.19e-16 at beta = 1.11, the bound the derivative series
accepts for degree 15.  The mode does three things:

  1. multi-start search in double precision (Levenberg-Marquardt on b_k k!, starts = today's set with c2 dropped, every
     entry scaled by a log-normal factor and its sign flipped with probability 1/4).  The system has the symmetry
     (c1, c3, c4, c5, c6, c10, c13) -> -(...), which gives the same polynomial: solutions are normalised to c1 > 0;
  2. every branch is polished by Newton in 80 digits and its rounding error in double precision is measured like
     tools/t16_rounding.py does (random Hermitian N = 64, spectral radius beta, three matrices, 80-bit reference).  Selection:
     among the branches within a factor 1.25 of the smallest max element error, the one with the smallest max |c_i|;
  3. the selected branch is printed as #define lines for grape_t18_coeffs.h, with its segment error.

Run:  python3 tools/t16_coeffs.py q [beta = 1.11] [starts = 500] [seed = 1]
"""
import sys
from mpmath import mp, mpf, mpc, matrix, lu_solve, besselj, factorial, chebyt, taylor, exp

sys.path.insert(0, __file__.rsplit("/", 1)[0])
from t18_coeffs import padd, pmul, mono   # noqa: E402

mp.dps = 80
NPAR = 16
# Taylor solution found by tools-internal multi-start Levenberg-Marquardt on the scaled system (x -> x/5), 16 digits
START = ["4.0187616102010362e-04", "2.9455314402796816e-03", "-8.7090665768376745e-03", "4.0175684406735668e-01",
         "3.2307628881223155e-02", "5.7689885130261453e+00", "2.3385760342712798e-02", "2.3810703738709912e-01",
         "2.2242091724963724e+00", "-5.7923617070732600e+00", "-4.1302763659296138e-02", "1.0408017352313534e+01",
         "-6.3317124558833640e+01", "3.4846658633645583e-01", "1.0", "1.0"]


def scal(p, s):
    return [s * x for x in p]


def t16_poly(c):
    c1, c2, c3, c4, c5, c6, c7, c8, c9, c10, c11, c12, c13, c14, c15, c16 = c
    y0 = pmul(mono({2: mpf(1)}), mono({2: c1, 1: c2}))
    y1 = padd(pmul(padd(y0, mono({2: c3, 1: c4})), padd(y0, mono({2: c5}))), padd(scal(y0, c6), mono({2: c7})))
    p = pmul(padd(y1, mono({2: c8, 1: c9})), padd(padd(y1, scal(y0, c10)), mono({1: c11})))
    p = padd(p, padd(padd(scal(y1, c12), scal(y0, c13)), mono({2: c14, 1: c15, 0: c16})))
    return p + [mpf(0)] * (17 - len(p))


def solve(target_fn, v0, iters=80):
    """Newton on b_k(c) = target_fn(c)[k], k = 0..15."""
    v = list(v0)

    def f_of(v):
        t = target_fn(v)
        return [pc - tc for pc, tc in zip(t16_poly(v)[:16], t)]
    for it in range(iters):
        f = f_of(v)
        err = max(abs(x) for x in f)
        if err < mpf(10) ** (-70):
            return v, err
        J = matrix(16, 16)
        h = mpf(10) ** (-40)
        for j in range(16):
            vp = list(v); vp[j] += h
            vm = list(v); vm[j] -= h
            fp, fm = f_of(vp), f_of(vm)
            for i in range(16):
                J[i, j] = (fp[i] - fm[i]) / (2 * h)
        dx = lu_solve(J, matrix(f))
        for j in range(16):
            v[j] -= dx[j]
    raise RuntimeError("no convergence, residual %s" % err)


def cheb_monomials(beta, deg):
    """Monomial coefficients in x = -i lam (real) of the degree-`deg` Chebyshev truncation of exp on |lam| <= beta."""
    lamc = [mpc(0)] * (deg + 1)
    for k in range(deg + 1):
        ck = (1 if k == 0 else 2) * (mpc(0, -1) ** k) * besselj(k, beta)
        for j, t in enumerate(taylor(lambda y: chebyt(k, y), 0, k)):
            lamc[j] += ck * t / mpf(beta) ** j
    out = []
    for j in range(deg + 1):
        tj = lamc[j] * mpc(0, 1) ** j
        assert abs(tj.imag) < mpf(10) ** (-60)
        out.append(tj.real)
    return out


def absorbed_x16(beta):
    """r_k, k = 0..15: x^16 - beta^16 2^-15 T_16(lam/beta) as a polynomial in x (lam = i x)."""
    tau = taylor(lambda y: chebyt(16, y), 0, 16)
    r = []
    for k in range(16):
        t = -(mpf(beta) ** (16 - k)) * tau[k] / mpf(2) ** 15 * (mpc(0, 1) ** k)
        assert abs(t.imag) < mpf(10) ** (-60)
        r.append(t.real)
    return r


def seg_error(v, beta, n=801):
    p = t16_poly(v)
    worst = mpf(0)
    for i in range(n):
        lam = -beta + 2 * beta * mpf(i) / (n - 1)
        x = mpc(0, -lam)
        acc = mpc(0)
        for c in reversed(p):
            acc = acc * x + c
        worst = max(worst, abs(acc - exp(x)))
    return worst


# ---- mode q: c2 = 0 --------------------------------------------------------------------------------------------------
QIDX = [0] + list(range(2, 16))        # positions of c1, c3..c16 in the full parameter list


def q_full(u):
    """c1, c3..c16 -> c1..c16 with c2 = 0"""
    v = [mpf(0)] * 16
    for i, x in zip(QIDX, u):
        v[i] = x
    return v


def q_target(beta):
    q14, r = cheb_monomials(beta, 14), absorbed_x16(beta)[:15]
    return lambda u: [b - u[0] ** 4 * rr for b, rr in zip(q14, r)]


def solve_q(target_fn, u0, iters=80):
    """Newton on b_k(c1, 0, c3..c16) = target_fn(u)[k], k = 0..14 (b_15 = 0 identically)."""
    u = [mpf(x) for x in u0]

    def f_of(u):
        p = t16_poly(q_full(u))
        assert p[15] == 0
        return [pc - tc for pc, tc in zip(p[:15], target_fn(u))]
    for it in range(iters):
        f = f_of(u)
        err = max(abs(x) for x in f)
        if err < mpf(10) ** (-70):
            return u, err
        J = matrix(15, 15)
        h = mpf(10) ** (-40)
        for j in range(15):
            up = list(u); up[j] += h
            um = list(u); um[j] -= h
            fp, fm = f_of(up), f_of(um)
            for i in range(15):
                J[i, j] = (fp[i] - fm[i]) / (2 * h)
        dx = lu_solve(J, matrix(f))
        for j in range(15):
            u[j] -= dx[j]
    raise RuntimeError("no convergence, residual %s" % err)


def q_search(beta, starts=500, seed=1, log=None):
    """the real branches of the c2 = 0 system the multi-start search reaches, as lists of 15 doubles with c1 > 0"""
    import numpy as np
    from numpy.polynomial import polynomial as P
    from scipy.optimize import least_squares
    q14 = np.array([float(x) for x in cheb_monomials(beta, 14)])
    r = np.array([float(x) for x in absorbed_x16(beta)[:15]])
    fact = np.array([float(factorial(k)) for k in range(15)])
    hdr = open(__file__.rsplit("/", 2)[0] + "/grape.jl_amd/csrc/grape_t18_coeffs.h").read()
    import re
    cur = np.array([float(re.search(r"#define\s+T16_C%d\s+(\S+)" % (i + 1), hdr).group(1)) for i in QIDX])

    def add(*ps):
        o = np.zeros(max(len(p) for p in ps))
        for p in ps:
            o[:len(p)] += p
        return o

    def res(u):
        c1, c3, c4, c5, c6, c7, c8, c9, c10, c11, c12, c13, c14, c15, c16 = u
        A, A2, y0 = np.array([0, 1.0]), np.array([0, 0, 1.0]), np.array([0, 0, 0, 0, c1])
        y1 = add(P.polymul(add(y0, c3 * A2, c4 * A), add(y0, c5 * A2)), c6 * y0, c7 * A2)
        p = add(P.polymul(add(y1, c8 * A2, c9 * A), add(y1, c10 * y0, c11 * A)), c12 * y1, c13 * y0, c14 * A2, c15 * A, [c16])
        return (p[:15] - (q14 - c1 ** 4 * r)) * fact

    flip = np.array([i in (0, 2, 3, 4, 5, 9, 12) for i in QIDX])        # the symmetry of the system (module text)
    rng = np.random.default_rng(seed)
    sols = []
    for s in range(starts):
        u0 = cur * np.exp(rng.normal(0, 1.0, 15)) * np.where(rng.random(15) < 0.25, -1, 1)
        try:
            o = least_squares(res, u0, method="lm", x_scale="jac", max_nfev=3000, xtol=1e-15, ftol=1e-15, gtol=1e-15)
        except Exception:
            continue
        if not np.isfinite(o.x).all() or np.abs(o.fun).max() > 1e-9:
            continue
        x = np.where(flip & (o.x[0] < 0), -o.x, o.x)
        if not any(np.allclose(x, y, rtol=1e-5, atol=1e-9) for y in sols):
            sols.append(x)
            if log:
                log("// start %d: new branch c1 = %.6e, c12 = %.4g, c13 = %.4g" % (s, x[0], x[10], x[11]))
    return [list(x) for x in sols]


def q_rounding(sets, beta, N=64):
    """max element error and 2-norm error in double precision of each full set at spectral radius beta (t16_rounding.py)"""
    import numpy as np
    import t16_rounding as R
    rng = np.random.default_rng(0)
    e = np.zeros((len(sets), 2))
    for _ in range(3):
        X = rng.normal(size=(N, N)) + 1j * rng.normal(size=(N, N)); H = X + X.conj().T
        H *= float(beta) / np.abs(np.linalg.eigvalsh(H)).max()
        A = -1j * H; U = R.reference(A)
        for i, c in enumerate(sets):
            D = (R.t16(A, c) - U).astype(np.complex128)
            e[i] = np.maximum(e[i], [np.abs(D).max(), np.linalg.norm(D, 2)])
    return e


def main_q(argv):
    beta = mpf(argv[0]) if len(argv) > 0 else mpf("1.11")
    starts = int(argv[1]) if len(argv) > 1 else 500
    seed = int(argv[2]) if len(argv) > 2 else 1
    tgt = q_target(beta)
    found = q_search(beta, starts, seed, log=print)
    branches = []
    for x in found:
        try:
            u, err = solve_q(tgt, x)
        except RuntimeError:
            continue
        if max(abs(a - b) for a, b in zip(u, x)) < mpf(10) ** (-6):
            branches.append(u)
    rnd = q_rounding([[float(x) for x in q_full(u)] for u in branches], beta)
    best = min(e[0] for e in rnd)
    for u, e in zip(branches, rnd):
        print("// branch c1 = %s, max |c| = %s: segment error %s, fp64 element error %.2e, 2-norm %.2e at rho = %s" %
              (mp.nstr(u[0], 8), mp.nstr(max(abs(x) for x in u), 5), mp.nstr(seg_error(q_full(u), beta), 4), e[0], e[1], mp.nstr(beta, 4)))
    ok = [u for u, e in zip(branches, rnd) if e[0] <= 1.25 * best]
    u = min(ok, key=lambda u: max(abs(x) for x in u))
    print("// selected: %d branches, %d within 1.25 of the best rounding; b16 * 16! = %s" %
          (len(branches), len(ok), mp.nstr(u[0] ** 4 * factorial(16), 5)))
    print("#define T16Q_THETA %s" % mp.nstr(beta, 5))
    for i, x in zip(QIDX, u):
        if i == 2:
            print("#define T16Q_C2 0.0")
        print("#define T16Q_C%d %s" % (i + 1, mp.nstr(x, 20)))
    return u


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "q":
        main_q(sys.argv[2:])
        return
    beta = mpf(sys.argv[1]) if len(sys.argv) > 1 else None
    v0 = [mpf(s) for s in START]
    tt = [1 / factorial(k) for k in range(16)]
    vt, err = solve(lambda v: tt, v0)
    print("// Taylor target: residual %s, shift of the start values %s, b16 * 16! = %s" %
          (mp.nstr(err, 3), mp.nstr(max(abs(a - b) for a, b in zip(vt, v0)), 3), mp.nstr(vt[0] ** 4 * factorial(16), 8)))
    sets = [("taylor", vt, mpf("0.7"))]
    if beta is not None:
        q15, r = cheb_monomials(beta, 15), absorbed_x16(beta)
        v = vt
        steps = 20
        for s in range(1, steps + 1):   # continuation from the Taylor solution
            w = mpf(s) / steps
            v, err = solve(lambda u: [a + w * (b - u[0] ** 4 * rr - a) for a, b, rr in zip(tt, q15, r)], v)
        print("// Chebyshev target on [-%s, %s]: residual %s, b16 * 16! = %s" %
              (mp.nstr(beta, 4), mp.nstr(beta, 4), mp.nstr(err, 3), mp.nstr(v[0] ** 4 * factorial(16), 8)))
        sets.append(("cheb", v, beta))
    for name, v, b in sets:
        print("// %s: max |p(-i lam) - exp(-i lam)| on |lam| <= %s: %s" % (name, mp.nstr(b, 4), mp.nstr(seg_error(v, b), 3)))
        print("static const double t16_%s[16] = {   // c1..c16" % name)
        print("    " + ",\n    ".join(mp.nstr(x, 20) for x in v) + "};")


if __name__ == "__main__":
    main()
