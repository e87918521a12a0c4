"""grape_hvp / grape_get_hvp_info without a GPU: the entry points exist in the header, the library, the ctypes binding and the
Julia glue, the ABI version did not move, a NULL handle is refused before anything touches HIP, ``GrapeHip.hvp`` handles the
shapes of V, and ``optimize(method="trust-ncg" | "newton-cg")`` drives ``hessp`` correctly (with a stub backend)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grape_hvp", "grape_get_hvp_info")


def _header():
    return open(os.path.join(ROOT, "include", "grape_hip.h")).read()


def test_entry_points_are_declared_exported_bound_and_called_from_julia():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+grape_hvp\s*\(\s*grape_handle\s*\*\s*h\s*,\s*int\s+nv\s*,\s*const\s+double\s*\*\s*V\s*,\s*double\s*\*\s*HV\s*\)\s*;", code)
    assert re.search(r"int\s+grape_get_hvp_info\s*\(\s*grape_handle\s*\*\s*h\s*,\s*double\s*\*\s*out\s*,\s*int\s+n\s*\)\s*;", code)
    assert re.search(r"#define\s+GRAPE_HIP_ABI_VERSION\s+7\b", _header()) and api.ABI_VERSION == 7
    lib = ctypes.CDLL(api.library_path())
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert re.search(r"ccall\(\(:" + name + r",\s*libgrape\)", jl), name
    assert "function hvp!(" in jl and "function hvp_info(" in jl
    assert hasattr(api.GrapeHip, "hvp") and hasattr(api.GrapeHip, "hvp_info")
    srcs, _ = api._sources()
    assert any(os.path.basename(s) == "grape_hvp.hip.h" for s in srcs)    # (a change of the new header rebuilds the library)


def test_null_handle_is_refused_without_touching_hip():
    from grape_jl_amd import api
    lib = api.load_library()
    v, hv, out = np.ones(4), np.full(4, 7.0), np.full(5, 7.0)
    assert lib.grape_hvp(None, 1, v.ctypes.data, hv.ctypes.data) == -1
    assert b"grape_hvp" in lib.grape_last_error(None)
    assert lib.grape_get_hvp_info(None, out.ctypes.data, 5) == -1
    assert (hv == 7.0).all() and (out == 7.0).all()


class _FakeLib:
    """stands in for the C library behind GrapeHip.hvp: records the call, returns 2 V"""

    def __init__(self):
        self.calls = []

    def grape_hvp(self, h, nv, vptr, outptr):
        n = self.LN * nv
        v = np.ctypeslib.as_array(ctypes.cast(vptr, ctypes.POINTER(ctypes.c_double)), shape=(n,))
        out = np.ctypeslib.as_array(ctypes.cast(outptr, ctypes.POINTER(ctypes.c_double)), shape=(n,))
        out[:] = 2.0 * v
        self.calls.append(nv)
        return 0


def test_shape_handling_of_hvp():
    from grape_jl_amd import api
    h = api.GrapeHip.__new__(api.GrapeHip)          # no handle, no device: only the argument handling is exercised
    h.L, h.N_T, h._h = 2, 3, None
    h._lib = _FakeLib()
    h._lib.LN = 6
    v1 = np.arange(6.0)
    out = h.hvp(v1)
    assert out.shape == (6,) and np.array_equal(out, 2 * v1)
    V = np.arange(18.0).reshape(3, 6)
    out = h.hvp(V[:, ::-1])                          # (not contiguous: copied before the pointer is taken)
    assert out.shape == (3, 6) and np.array_equal(out, 2 * V[:, ::-1])
    out = h.hvp([[1, 2, 3, 4, 5, 6]])                # a list of integers
    assert out.shape == (1, 6) and out.dtype == np.float64
    assert h._lib.calls == [1, 3, 1]
    for bad in (np.zeros(5), np.zeros((2, 5)), np.zeros((0, 6)), np.zeros((1, 1, 6)), 1.0):
        with pytest.raises(ValueError):
            h.hvp(bad)
    assert h._lib.calls == [1, 3, 1]


class _QuadraticBackend:
    """J(x) = 1/2 (x - x*)^T A (x - x*) behind the backend interface of grape.py; like the device, `hvp` answers at the point
    of the last evaluation and refuses when there is none"""

    def __init__(self, A, xstar):
        self.A, self.xstar, self.x_last = A, xstar, None
        self.n_eval = self.n_grad = self.n_hvp = 0
        self.K, self.functional, self.K_total, self.lambda_b = 1, 0, 1, 0.0

    def eval(self, x, gradient=True, want_psiT=False):
        x = np.array(x, dtype=float)
        self.x_last = x
        self.n_eval += 1
        self.n_grad += bool(gradient)
        d = x - self.xstar
        J, G = 0.5 * d @ self.A @ d, (self.A @ d if gradient else None)
        self.J_last = float(J)
        self.J_first = getattr(self, "J_first", float(J))
        self.J_best = min(getattr(self, "J_best", np.inf), float(J))
        tau = np.array([1.0 + 0j])
        psiT = np.zeros((1, 2), complex)
        return (J, G, tau, psiT) if want_psiT else (J, G, tau)

    def hvp(self, V):
        assert self.x_last is not None, "no valid forward state"
        self.n_hvp += 1
        return np.asarray(V) @ self.A


def _stub_problem():
    from grape_jl_amd import grape as G
    H = G.hamiltonian(np.diag([1.0, -1.0]), (np.array([[0, 1], [1, 0]], complex), lambda t: 0.1))
    tlist = np.linspace(0, 1, 7)
    traj = G.Trajectory(np.array([1, 0], complex), H, target_state=np.array([0, 1], complex))
    rng = np.random.default_rng(3)
    M = rng.normal(size=(6, 6))
    return G, [traj], tlist, M @ M.T + 6 * np.eye(6), rng.normal(size=6)


@pytest.mark.parametrize("method", ["trust-ncg", "newton-cg"])
def test_hessp_plumbing_of_optimize(method):
    G, trajs, tlist, A, xstar = _stub_problem()
    be = _QuadraticBackend(A, xstar)
    # (optimize takes the value of J_T from the host-side functional: it reports what the stub computed last)
    res = G.optimize(trajs, tlist, backend=be, J_T=lambda Psi, tr, tau=None: be.J_last, method=method, iter_stop=50,
                     rethrow_exceptions=True, solver_options=dict(gtol=1e-10) if method == "trust-ncg" else dict(xtol=1e-12))
    assert not res.message.startswith("Exception"), res.message
    assert be.n_hvp > 0 and be.n_grad > 0
    # a quadratic is minimised by Newton steps: the solver gets there only if hessp returns A p, at the right point
    print(method, dict(J_first=be.J_first, J_best=be.J_best, evals=be.n_eval, hvps=be.n_hvp, iters=res.iter))
    assert be.J_first > 1.0 and be.J_best <= 1e-12 * be.J_first
    assert res.iter >= 1 and res.J_T <= 1e-12 * be.J_first


def test_hessp_reevaluates_when_the_last_evaluation_was_elsewhere():
    G, trajs, tlist, A, xstar = _stub_problem()
    be = _QuadraticBackend(A, xstar)
    wrk = G.GrapeWrk(trajs, tlist, backend=be, J_T=lambda Psi, tr, tau=None: 0.0)
    state = {}
    hessp = G._make_hessp(wrk, None, state)
    p = np.arange(6.0)
    x0 = np.zeros(6)
    assert np.allclose(hessp(x0, p), A @ p)             # nothing evaluated yet: the forward half runs first
    assert be.n_eval == 1 and be.n_grad == 0 and np.array_equal(be.x_last, x0)
    hessp(x0, p)
    assert be.n_eval == 1                               # same point: no second evaluation
    be.eval(np.ones(6))
    state["x_eval"] = np.ones(6)                        # what fg leaves behind after a rejected trial step at another point
    assert np.allclose(hessp(x0, p), A @ p)
    assert be.n_eval == 3 and be.n_grad == 1 and np.array_equal(be.x_last, x0)
    assert state["hessp_calls"] == 3


def test_second_order_methods_refuse_what_they_cannot_differentiate():
    G, trajs, tlist, A, xstar = _stub_problem()
    J_T = lambda Psi, tr, tau=None: 0.0   # noqa: E731

    class NoHvp:
        eval = _QuadraticBackend.eval

    with pytest.raises(ValueError, match="hvp"):
        G.optimize(trajs, tlist, backend=NoHvp(), J_T=J_T, method="trust-ncg")
    with pytest.raises(ValueError, match="J_a"):
        G.optimize(trajs, tlist, backend=_QuadraticBackend(A, xstar), J_T=J_T, method="newton-cg", J_a=lambda x, t: 0.0)
    with pytest.raises(ValueError, match="bounds"):
        G.optimize(trajs, tlist, backend=_QuadraticBackend(A, xstar), J_T=J_T, method="trust-ncg", upper_bound=1.0)
    with pytest.raises(ValueError, match="method"):
        G.optimize(trajs, tlist, backend=_QuadraticBackend(A, xstar), J_T=J_T, method="bfgs")
