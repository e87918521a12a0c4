"""Host-side mirror of the reference interface (grape.jl_amd/grape.py), CPU only.  The evaluator
behind fg! is injected: here the oracle stands in for the HIP library so that the optimizer loop,
result bookkeeping and error behaviour can be checked without a GPU."""
import os

import numpy as np
import pytest

import grape_oracle as go
from grape_jl_amd import grape as G


class OracleBackend:
    """Test stand-in with the GrapeHip.eval signature (tests may use the oracle as the checker)."""

    def __init__(self, wrk_args):
        self.a = wrk_args

    def eval(self, pulsevals, gradient=True, want_psiT=False):
        H0, Hc, tl, p0, tg = self.a
        if gradient:
            J, g, tau, parts = go.evaluate_gradient(H0, Hc, tl, pulsevals, p0, tg, return_parts=True)
            psiT = parts["storage"][:, -1]
        else:
            J, tau, st = go.evaluate_functional(H0, Hc, tl, pulsevals, p0, tg)
            g, psiT = None, st[:, -1]
        return (J, g, tau, psiT) if want_psiT else (J, g, tau)


def tls(eps, nt=101):
    sz = np.array([[-0.5, 0], [0, 0.5]], complex)
    sx = np.array([[0, 1], [1, 0]], complex)
    H = G.hamiltonian(sz, (sx, eps))
    tlist = np.linspace(0, 5, nt)
    traj = G.Trajectory(np.array([1, 0], complex), H, target_state=np.array([0, 1], complex))
    be = OracleBackend((sz[None], sx[None], tlist, np.array([[1, 0]], complex), np.array([[0, 1]], complex)))
    return [traj], tlist, be


def test_discretize_midpoints_roundtrip():
    tl = np.linspace(0, 1, 6)
    v = G.discretize_on_midpoints(lambda t: t, tl)
    assert len(v) == 5 and v[0] == 0.0 and v[-1] == 1.0 and abs(v[2] - 0.5) < 1e-15
    on_pts = G.discretize(v, tl)
    assert len(on_pts) == 6 and on_pts[0] == v[0] and on_pts[-1] == v[-1]
    assert np.allclose(G.discretize_on_midpoints(np.arange(6.0), tl), [0, 1.5, 2.5, 3.5, 5][:5][:5])


def test_no_controls_and_missing_J_T():
    sz = np.diag([1.0, -1.0]).astype(complex)
    traj = G.Trajectory(np.array([1, 0], complex), G.hamiltonian(sz), target_state=np.array([0, 1], complex))
    with pytest.raises(ValueError, match="no controls"):
        G.GrapeWrk([traj], np.linspace(0, 1, 5), backend=object(), J_T=G.J_T_sm)
    trajs, tl, be = tls(lambda t: 0.2)
    with pytest.raises(ValueError, match="J_T"):
        G.GrapeWrk(trajs, tl, backend=be)


def test_optimize_tls_reaches_reference_thresholds():
    # behaviour pinned by /root/reference/test/test_tls_optimization.jl:148-173:
    # flattop * 0.2 guess, J_T_sm, <= 5 L-BFGS-B iterations -> J_T < 1e-3 and 0.75 < max|eps| < 0.85
    def guess(t, T=5.0, t_rise=0.3):
        f = 1.0
        if t < t_rise:
            f = np.sin(np.pi * t / (2 * t_rise)) ** 2
        elif t > T - t_rise:
            f = np.sin(np.pi * (t - T) / (2 * t_rise)) ** 2
        return 0.2 * f
    trajs, tl, be = tls(guess, nt=101)
    seen = []
    res = G.optimize(trajs, tl, backend=be, J_T=G.J_T_sm, iter_stop=5,
                     callback=lambda wrk, it: seen.append((it, wrk.result.J_T)) or (it, wrk.result.J_T))
    assert res.J_T < 1e-3
    assert 0.75 < np.max(np.abs(res.optimized_controls[0])) < 0.85
    assert res.iter <= 5 and res.fg_calls >= res.iter + 1
    assert seen[0][0] == 0 and len(res.records) == len(seen)
    assert res.converged or "CONVERGENCE" in res.message.upper() or "Reached" in res.message


def test_check_convergence_string_and_bounds():
    trajs, tl, be = tls(lambda t: 0.2, nt=51)
    res = G.optimize(trajs, tl, backend=be, J_T=G.J_T_sm, iter_stop=50, upper_bound=0.7, lower_bound=-0.7,
                     check_convergence=lambda r: "J_T < 10^-2" if r.J_T < 1e-2 else "")
    assert res.converged and res.message == "J_T < 10^-2"
    assert np.max(np.abs(res.optimized_controls[0])) < 0.700001  # test_tls_optimization.jl:260


def test_exception_is_captured_in_message():
    trajs, tl, _ = tls(lambda t: 0.2, nt=11)

    class Boom:
        def eval(self, *a, **k):
            raise RuntimeError("GRAPE_ERR_HIP: boom")
    res = G.optimize(trajs, tl, backend=Boom(), J_T=G.J_T_sm)
    assert res.message.startswith("Exception:") and "boom" in res.message  # src/optimize.jl:125-135
    with pytest.raises(RuntimeError):
        G.optimize(trajs, tl, backend=Boom(), J_T=G.J_T_sm, rethrow_exceptions=True)


def test_amplitude_wrapper_chain_rule_and_j_parts_split():
    """Host logic of the non-linear amplitudes (chain rule over the evaluator's gradient) and of the J_T / J_b
    bookkeeping, with the oracle standing in for the HIP library."""
    trajs, tl, be = tls(lambda t: 0.2, nt=41)
    N_T = len(tl) - 1
    A = 0.5
    wrapped = G._AmplitudeBackend(be, [lambda e: A * np.tanh(e / A)], [lambda e: 1.0 / np.cosh(e / A) ** 2], N_T)
    x = 0.4 + 0.1 * np.sin(np.arange(N_T))
    J, g, tau = wrapped.eval(x)
    for idx in (0, 17, N_T - 1):
        xp, xm = x.copy(), x.copy()
        xp[idx] += 1e-6
        xm[idx] -= 1e-6
        fd = (wrapped.eval(xp, gradient=False)[0] - wrapped.eval(xm, gradient=False)[0]) / 2e-6
        assert abs(fd - g[idx]) <= 1e-8
    # the amplitudes the evaluator sees never exceed the saturation value
    assert np.abs(wrapped._map(x * 100, wrapped.funcs)).max() <= A
    # J_parts: J_T from tau, nothing attributed to a state running cost that is not there
    wrk = G.GrapeWrk(trajs, tl, backend=be, J_T=G.J_T_sm)
    Gv = np.zeros(N_T)
    Jtot = G.evaluate_gradient_b(Gv, wrk.pulsevals, wrk)
    assert abs(wrk.J_parts[0] - Jtot) <= 1e-14 and wrk.J_parts[2] == 0.0
    G.update_result(wrk, 0)
    assert wrk.result.J_b == 0.0 and abs(wrk.result.J_T - Jtot) <= 1e-14


def test_iteration_table_mirrors_the_reference_format():
    # make_grape_print_iters, /root/reference/src/optimize.jl:310-537: header row in iteration 0, "n/a" for differences
    # there, %.2e numbers, FG(F) as fg(f), records of the stored fields
    import io
    trajs, tl, be = tls(lambda t: 0.2, nt=51)
    buf = io.StringIO()
    cb = G.make_grape_print_iters(store_iter_info=("iter.", "J_T", "ǁ∇Jǁ"), out=buf)
    res = G.optimize(trajs, tl, backend=be, J_T=G.J_T_sm, iter_stop=3, callback=cb)
    lines = buf.getvalue().splitlines()
    assert lines[0].split() == ["iter.", "J_T", "ǁ∇Jǁ", "ǁΔϵǁ", "ΔJ", "FG(F)", "secs"]
    assert len(lines) == 1 + len(res.records) == 1 + res.iter + 1
    first = lines[1].split()
    assert first[0] == "0" and first[3] == "n/a" and first[4] == "n/a" and first[5] == "1(0)"
    assert all(len(ln) == 6 + 4 * 11 + 8 + 8 for ln in lines)
    assert res.records[0][0] == 0 and abs(res.records[-1][1] - res.J_T) < 1e-15
    import re
    assert re.fullmatch(r"-?\d\.\d\de[+-]\d\d", lines[2].split()[1])
    with pytest.raises(ValueError):
        G.make_grape_print_iters(print_iter_info=("iter.", "∠°"))


def test_iter_start_stop_and_callback_chain():
    # /root/reference/test/test_iterations.jl:18-41 (records of iterations [0, 11, 12] with iter_start = 10) and :43-125
    # (a tuple of callbacks is called in order, their return values are concatenated with the stored table fields)
    import io
    trajs, tl, be = tls(lambda t: 0.2, nt=31)
    buf = io.StringIO()
    res = G.optimize(trajs, tl, backend=be, J_T=G.J_T_ss, iter_start=10, iter_stop=12, store_iter_info=("iter.", "J_T"),
                     print_iters_out=buf)
    assert res.converged and res.iter_start == 10 and res.iter_stop == 12
    assert [r[0] for r in res.records] == [0, 11, 12]
    assert buf.getvalue().splitlines()[0].split()[0] == "iter."
    calls = []

    def cb1(wrk, it, *a):
        calls.append(("cb1", it))

    def cb2(wrk, it, *a):
        calls.append(("cb2", it))
        return ("cb2", it)
    res = G.optimize(trajs, tl, backend=be, J_T=G.J_T_ss, iter_stop=1, callback=(cb1, cb2))
    assert res.converged and calls == [("cb1", 0), ("cb2", 0), ("cb1", 1), ("cb2", 1)]
    assert res.records == [("cb2", 0), ("cb2", 1)]
    res = G.optimize(trajs, tl, backend=be, J_T=G.J_T_ss, iter_stop=1, callback=(cb1, cb2), store_iter_info=("J_T",),
                     print_iters=False)
    assert len(res.records) == 2 and len(res.records[0]) == 3 and res.records[0][:2] == ("cb2", 0)
    assert isinstance(res.records[0][2], float)


def test_continue_from_previous_result():
    # src/workspace.jl:167-186 (test/test_tls_optimization.jl:417-480 continues across methods; here GRAPE -> GRAPE):
    # the result object is reused, iterations keep counting, the first J_T of the continuation is the last of the first run
    trajs, tl, be = tls(lambda t: 0.2, nt=51)
    r1 = G.optimize(trajs, tl, backend=be, J_T=G.J_T_sm, iter_stop=2, store_iter_info=("iter.", "J_T"), print_iters=False)
    J_mid, n_rec = r1.J_T, len(r1.records)
    assert r1.iter == 2 and r1.message == "Reached maximum number of iterations"
    r2 = G.optimize(trajs, tl, backend=be, J_T=G.J_T_sm, iter_stop=5, continue_from=r1, store_iter_info=("iter.", "J_T"),
                    print_iters=False)
    assert r2 is r1 and r2.iter == 5 and r2.iter_stop == 5 and r2.J_T < J_mid
    # iteration 0 of the continuation re-evaluates the pulses re-discretised from the optimized controls (on tlist):
    # intervals -> points -> midpoints is not the identity, so J_T is close to, not equal to, the last value
    assert abs(r2.records[n_rec][1] - J_mid) < 0.05 * J_mid and r2.records[n_rec][0] == 0
    assert [r[0] for r in r2.records[n_rec + 1:]] == [3, 4, 5]


class OracleBackendWithStorage(OracleBackend):
    """... that also keeps the stored states, as GrapeHip.storage hands them out"""

    def eval(self, pulsevals, gradient=True, want_psiT=False):
        H0, Hc, tl, p0, tg = self.a
        if gradient:
            J, g, tau, parts = go.evaluate_gradient(H0, Hc, tl, pulsevals, p0, tg, return_parts=True)
            self.fw, self.bw = parts["storage"], np.concatenate([parts["chi"], parts["chi"][:, -1:]], axis=1)
            psiT = parts["storage"][:, -1]
        else:
            J, tau, st = go.evaluate_functional(H0, Hc, tl, pulsevals, p0, tg)
            self.fw, self.bw = st, None
            g, psiT = None, st[:, -1]
        return (J, g, tau, psiT) if want_psiT else (J, g, tau)

    def storage(self, which=0):
        return self.fw if which == 0 else self.bw

    def set_fused_sweeps(self, on):
        self.fused = on
        return False


def test_propagation_callbacks_are_synthesised_from_the_stored_states():
    """per-step propagation callbacks (/root/reference/src/optimize.jl:733-737 forward, :882-887 / :973-978 backward): on the HIP path
    the steps do not run on the host, the mirror calls `prop_callback(propagator, observables)` afterwards from the stored
    states -- once per time step, in time order forward and in reverse order backward, with the state just reached"""
    trajs, tl, _ = tls(lambda t: 0.3, nt=21)
    seen = []
    trajs[0].prop_callback = lambda prop, obs: seen.append((prop.backward, prop.n, prop.t, prop.state.copy(), obs))
    trajs[0].prop_observables = "obs"
    sz = np.array([[-0.5, 0], [0, 0.5]], complex)
    sx = np.array([[0, 1], [1, 0]], complex)
    be = OracleBackendWithStorage((sz[None], sx[None], tl, np.array([[1, 0]], complex), np.array([[0, 1]], complex)))
    wrk = G.GrapeWrk(trajs, tl, backend=be, J_T=G.J_T_sm)
    assert be.fused is False                                   # sequential sweeps while callbacks are registered
    G.evaluate_functional(wrk.pulsevals, wrk)
    N_T = len(tl) - 1
    assert [s[1] for s in seen] == list(range(1, N_T + 1)) and not any(s[0] for s in seen) and all(s[4] == "obs" for s in seen)
    assert all(abs(s[2] - tl[s[1]]) < 1e-15 for s in seen)
    assert np.allclose(seen[-1][3], wrk._states[0]) and np.allclose(seen[3][3], be.fw[0, 4])
    assert all(abs(np.linalg.norm(s[3]) - 1.0) < 1e-12 for s in seen)
    seen.clear()
    Gout = np.zeros_like(wrk.pulsevals)
    G.evaluate_gradient_b(Gout, wrk.pulsevals, wrk)
    fwd = [s for s in seen if not s[0]]
    bwd = [s for s in seen if s[0]]
    assert [s[1] for s in fwd] == list(range(1, N_T + 1)) and [s[1] for s in bwd] == list(range(N_T - 1, -1, -1))
    assert seen.index(bwd[0]) > seen.index(fwd[-1])            # the backward calls follow the forward ones
    assert np.allclose(bwd[0][3], be.bw[0, N_T - 1]) and np.allclose(bwd[-1][3], be.bw[0, 0])


def test_bench_gpus_flag_and_world_size_must_agree(tmp_path):
    """bench.py --gpus N under a launcher that set another WORLD_SIZE is refused before torch is imported (no GPU needed):
    the JSON line may never carry an n_gpus the caller did not ask for"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "1"], capture_output=True,
                         text=True, timeout=60, env=env)
    assert res.returncode == 2 and not res.stdout.strip() and "WORLD_SIZE=4" in res.stderr


def test_bench_refuses_a_run_without_timed_steps():
    """bench.py --steps 0 is refused before torch is imported (no GPU needed): ms_per_step would have no steps to divide"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True,
                         text=True, timeout=60, env=env)
    assert res.returncode == 2 and not res.stdout.strip() and "--steps" in res.stderr
