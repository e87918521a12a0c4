"""grape_hessian / grape_get_hessian_info without a GPU: the entry points exist in the header, the library, the ctypes binding
and the Julia glue, the ABI version did not move, a NULL handle is refused before anything touches HIP,
``GrapeHip.hessian`` shapes its result, and ``optimize(method="trust-exact")`` drives ``hess`` correctly (with a stub backend)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grape_hessian", "grape_get_hessian_info")


def _header():
    return open(os.path.join(ROOT, "include", "grape_hip.h")).read()


def test_entry_points_are_declared_exported_bound_and_called_from_julia():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+grape_hessian\s*\(\s*grape_handle\s*\*\s*h\s*,\s*double\s*\*\s*H\s*\)\s*;", code)
    assert re.search(r"int\s+grape_get_hessian_info\s*\(\s*grape_handle\s*\*\s*h\s*,\s*double\s*\*\s*out\s*,\s*int\s+n\s*\)\s*;", code)
    assert re.search(r"#define\s+GRAPE_HIP_ABI_VERSION\s+7\b", _header()) and api.ABI_VERSION == 7
    lib = ctypes.CDLL(api.library_path())
    assert lib.grape_abi_version() == 7
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert re.search(r"ccall\(\(:" + name + r",\s*libgrape\)", jl), name
    assert "function hessian!(" in jl and "function hessian_info(" in jl
    assert hasattr(api.GrapeHip, "hessian") and hasattr(api.GrapeHip, "hessian_info")
    srcs, _ = api._sources()
    assert any(os.path.basename(s) == "grape_hessian.hip.h" for s in srcs)    # (a change of the new header rebuilds the library)


def test_null_handle_is_refused_without_touching_hip():
    """(a NULL H needs a handle, and a handle a device: tests/test_gpu_hessian.py refuses it there)"""
    from grape_jl_amd import api
    lib = api.load_library()
    H, out = np.full(4, 7.0), np.full(8, 7.0)
    assert lib.grape_hessian(None, H.ctypes.data) == -1 and lib.grape_hessian(None, None) == -1
    assert lib.grape_last_error(None).startswith(b"grape_hessian:")
    assert lib.grape_get_hessian_info(None, out.ctypes.data, 8) == -1
    assert (H == 7.0).all() and (out == 7.0).all()


class _FakeLib:
    """stands in for the C library behind GrapeHip.hessian: fills H with its flat index, the info with 1..8"""

    def __init__(self, P):
        self.P, self.calls = P, 0

    def grape_hessian(self, h, outptr):
        out = np.ctypeslib.as_array(ctypes.cast(outptr, ctypes.POINTER(ctypes.c_double)), shape=(self.P * self.P,))
        out[:] = np.arange(self.P * self.P)
        self.calls += 1
        return 0

    def grape_get_hessian_info(self, h, outptr, n):
        out = np.ctypeslib.as_array(ctypes.cast(outptr, ctypes.POINTER(ctypes.c_double)), shape=(n,))
        out[:] = np.arange(1, n + 1)
        return n


def test_shape_handling_of_hessian():
    from grape_jl_amd import api
    h = api.GrapeHip.__new__(api.GrapeHip)          # no handle, no device: only the argument handling is exercised
    h.L, h.N_T, h._h = 2, 3, None
    h._lib = _FakeLib(6)
    H = h.hessian()
    assert H.shape == (6, 6) and H.dtype == np.float64 and H.flags["C_CONTIGUOUS"]
    assert np.array_equal(H, np.arange(36.0).reshape(6, 6))
    assert h._lib.calls == 1
    info = h.hessian_info()
    assert info == dict(series_terms=1, series_steps=2, traj_per_pass=3, bytes=4, ms=5.0, terms_forward_seeds=6,
                        terms_backward_seeds=7, terms_fan=8)


class _QuadraticBackend:
    """J(x) = 1/2 (x - x*)^T A (x - x*) behind the backend interface of grape.py; like the device, `hessian` answers at the
    point of the last evaluation and refuses when there is none"""

    def __init__(self, A, xstar):
        self.A, self.xstar, self.x_last = A, xstar, None
        self.n_eval = self.n_grad = self.n_hess = 0
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

    def hessian(self):
        assert self.x_last is not None, "no valid forward state"
        self.n_hess += 1
        return self.A.copy()


def _stub_problem():
    from grape_jl_amd import grape as G
    H = G.hamiltonian(np.diag([1.0, -1.0]), (np.array([[0, 1], [1, 0]], complex), lambda t: 0.1))
    tlist = np.linspace(0, 1, 7)
    traj = G.Trajectory(np.array([1, 0], complex), H, target_state=np.array([0, 1], complex))
    rng = np.random.default_rng(3)
    M = rng.normal(size=(6, 6))
    return G, [traj], tlist, M @ M.T + 6 * np.eye(6), rng.normal(size=6)


def test_hess_plumbing_of_optimize():
    G, trajs, tlist, A, xstar = _stub_problem()
    be = _QuadraticBackend(A, xstar)
    # (optimize takes the value of J_T from the host-side functional: it reports what the stub computed last)
    res = G.optimize(trajs, tlist, backend=be, J_T=lambda Psi, tr, tau=None: be.J_last, method="trust-exact", iter_stop=50,
                     rethrow_exceptions=True, solver_options=dict(gtol=1e-10))
    assert not res.message.startswith("Exception"), res.message
    assert be.n_hess > 0 and be.n_grad > 0
    # a quadratic is minimised by Newton steps: the solver gets there only if hess returns A, at the right point
    print(dict(J_first=be.J_first, J_best=be.J_best, evals=be.n_eval, hessians=be.n_hess, iters=res.iter))
    assert be.J_first > 1.0 and be.J_best <= 1e-12 * be.J_first
    assert res.iter >= 1 and res.J_T <= 1e-12 * be.J_first


def test_hess_reevaluates_when_the_last_evaluation_was_elsewhere():
    G, trajs, tlist, A, xstar = _stub_problem()
    be = _QuadraticBackend(A, xstar)
    wrk = G.GrapeWrk(trajs, tlist, backend=be, J_T=lambda Psi, tr, tau=None: 0.0)
    state = {}
    hess = G._make_hess(wrk, None, state)
    x0 = np.zeros(6)
    assert np.array_equal(hess(x0), A)                  # nothing evaluated yet: the forward half runs first
    assert be.n_eval == 1 and be.n_grad == 0 and np.array_equal(be.x_last, x0)
    hess(x0)
    assert be.n_eval == 1                               # same point: no second evaluation
    be.eval(np.ones(6))
    state["x_eval"] = np.ones(6)                        # what fg leaves behind after a rejected trial step at another point
    assert np.array_equal(hess(x0), A)
    assert be.n_eval == 3 and be.n_grad == 1 and np.array_equal(be.x_last, x0)
    assert state["hess_calls"] == 3


def test_trust_exact_refuses_what_it_cannot_differentiate():
    G, trajs, tlist, A, xstar = _stub_problem()
    J_T = lambda Psi, tr, tau=None: 0.0   # noqa: E731

    class NoHessian:
        eval = _QuadraticBackend.eval

    with pytest.raises(ValueError, match="hessian"):
        G.optimize(trajs, tlist, backend=NoHessian(), J_T=J_T, method="trust-exact")
    with pytest.raises(ValueError, match="J_a"):
        G.optimize(trajs, tlist, backend=_QuadraticBackend(A, xstar), J_T=J_T, method="trust-exact", J_a=lambda x, t: 0.0)
    with pytest.raises(ValueError, match="bounds"):
        G.optimize(trajs, tlist, backend=_QuadraticBackend(A, xstar), J_T=J_T, method="trust-exact", upper_bound=1.0)
