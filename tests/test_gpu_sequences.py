"""One long-lived handle, default settings, many calls -- needs an MI355X.

grape_eval with a gradient runs uncaptured twice, then replays ONE captured graph (every 16th call uncaptured again): an
optimizer spends nine evaluations in ten there, with getters, split-phase halves, Hessian-vector products and batches in
between.  Every step of the script (tests/sequence_inputs.py: SCRIPT) is compared with

  * a fresh twin: a new handle under GRAPE_GRAPH=0 that makes only the calls the step needs -- J, G, tau and every getter's
    output BIT FOR BIT (``np.array_equal``);
  * the existing references at their bars: the C oracle (|dJ|, |dtau| <= 1e-12 * scale, |dG| <= 1e-10 * max(|G|, 1e-3)),
    tests/hvp_reference.py (1e-10 * max(|Hv|, 1e-3)) and tests/frame_reference.py for dJ/d(dt_n) (1e-10 * max(|.|, 1e-3)).

The environment is a user's: GRAPE_DERIV3 (pinned by tests/conftest.py for the session) is removed, the graph is on.  A test
collects every deviation of its script and asserts once at the end, after printing the worst figure per reference."""
import numpy as np
import pytest

import frame_reference as fr
import hvp_reference as hr
import sequence_inputs as si

pytestmark = pytest.mark.gpu

HVP_REFERENCE_MAX_N = 32      # (a 4N x 4N exponential per cell, control and direction: seconds beyond; tests/test_gpu_hvp.py has N <= 64)


@pytest.fixture(scope="module")
def g():
    import grape_jl_amd as mod
    return mod


@pytest.fixture(autouse=True)
def default_environment(monkeypatch):
    monkeypatch.delenv("GRAPE_DERIV3", raising=False)
    monkeypatch.delenv("GRAPE_GRAPH", raising=False)


def same(a, b):
    """bit for bit; tuples and dicts element by element"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


def differing(a, b):
    """the keys in which two dicts of numbers differ, with both values"""
    return {k: (float(a[k]), float(b[k])) for k in a if not same(a[k], b[k])}


class Run:
    """the long-lived handle of a case, its twins, the oracle, and what deviated"""

    def __init__(self, g, ref, monkeypatch, cid, pr, with_D=False):
        self.g, self.ref, self.mp, self.cid, self.pr = g, ref, monkeypatch, cid, pr
        self.kw = dict(functional=pr.get("functional", 0))
        self.D = None
        if with_D:
            self.D = si.penalty(cid)
            self.kw.update(D=self.D, lambda_b=si.LAMBDA_B)
        self.bad, self.worst, self.next_pulse = [], {}, 0
        # the C oracle's exact gradient costs a second per call from N = 40 on: there it is asked at the steps marked
        # against_oracle=True only (every other evaluation still has the fresh handle's bits)
        self.heavy = pr["N"] >= 40
        self.h = self.create()

    def create(self, graph=True):
        pr = self.pr
        if not graph:
            self.mp.setenv("GRAPE_GRAPH", "0")               # (read once, in grape_create)
        try:
            return self.g.GrapeHip(pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"], pr["weights"], **self.kw)
        finally:
            self.mp.delenv("GRAPE_GRAPH", raising=False)

    def twin(self):
        return self.create(graph=False)

    def x(self):
        i = self.next_pulse
        self.next_pulse += 1
        return si.pulses(self.cid, i) if self.cid in si.CASES else si.part_a_pulses(i)

    def note(self, ok, what):
        if not ok:
            self.bad.append(what)

    def bar(self, key, dev, tol, what):
        dev = float(dev)
        w = self.worst.setdefault(key, [0.0, tol, what])
        if dev / tol >= w[0] / w[1]:
            self.worst[key] = [dev, tol, what]
        self.note(dev <= tol, f"{what}: {key} deviates by {dev:.3e}, bar {tol:.3e}")

    def scale(self, tau, psiT=None):
        """1 for normalised states; general generators do not keep the norm (tests/test_gpu_scan.py)"""
        s = max(1.0, float(np.abs(tau).max()))
        if psiT is not None:
            s = max(s, float(np.abs(psiT).max()))
        return s ** 2

    def oracle(self, x):
        pr = self.pr
        kw = dict(D=self.D, lambda_b=si.LAMBDA_B) if self.D is not None else {}
        method = self.ref.GRADGEN if pr["K"] * pr["N_T"] <= 400 else self.ref.TAYLOR
        return self.ref.evaluate(pr["H0"], pr["Hc"], pr["tlist"], x, pr["psi0"], pr["target"], pr["weights"],
                                 functional=self.kw["functional"], gradient_method=method, want_parts=True, **kw)

    def check_eval(self, what, x=None, h=None, against_oracle=None, work=True):
        """h.eval(x) against the twin's eval(x), bit for bit, and against the C oracle.  ``work``: grape_get_work as well -- the
        statistics are reset together with the flag word, so a reset that a replay got wrong shows there whatever the status"""
        x = self.x() if x is None else x
        try:
            got = (h or self.h).eval(x)
        except self.g.GrapeHipError as e:
            self.note(False, f"{what}: eval returned {e}")
            return x, None
        with self.twin() as t:
            want = t.eval(x)
            wt = t.work() if work else None
        if work:
            wh = (h or self.h).work()
            self.note(same(wh, wt), f"{what}: work() differs from the fresh handle's: {differing(wh, wt)}")
        self.note(same(got, want), f"{what}: eval differs from the fresh handle's in at least one bit "
                                   f"(J {got[0] - want[0]:.3e}, G {np.abs(got[1] - want[1]).max():.3e}, tau {np.abs(got[2] - want[2]).max():.3e})")
        if against_oracle or (against_oracle is None and not self.heavy):
            Jr, Gr, taur, parts = self.oracle(x)
            sc = self.scale(taur, parts["psiT"])
            self.bar("J vs oracle", abs(got[0] - Jr), 1e-12 * max(sc, abs(Jr)), what)
            self.bar("tau vs oracle", np.abs(got[2] - taur).max(), 1e-12 * sc, what)
            self.bar("G vs oracle", np.abs(got[1] - Gr).max(), 1e-10 * max(np.abs(Gr).max(), 1e-3), what)
        return x, got

    def getter(self, h, name):
        pr = self.pr
        if name == "final_states":
            return h.final_states()
        if name == "sums":
            return h.sums()
        if name in ("storage0", "storage1"):
            return h.storage(int(name[-1]))
        if name == "tau_grads":
            return h.tau_grads()
        if name == "propagator":
            return h.propagator(pr["K"] - 1, pr["N_T"] - 1)
        if name == "work":
            return h.work()
        if name == "timings":
            t = h.timings()
            assert set(t) >= {"expm", "forward", "backward", "deriv", "reduce", "total"}
            return None                                          # (milliseconds: nothing to compare)
        if name == "time_gradient":
            return h.time_gradient()
        raise KeyError(name)

    def report(self):
        for key, (dev, tol, what) in sorted(self.worst.items()):
            print(f"{self.cid}: worst {key}: {dev:.3e} (bar {tol:.3e}) at {what}")
        for b in self.bad:
            print("DEVIATION", self.cid, b)
        assert not self.bad, self.bad


def kernels_asserted(run, w):
    """the kernels of the default route, from grape_get_work"""
    c = si.CASES[run.cid]
    N, herm = c["N"], c["herm"]
    want_asm = 0
    if N >= 49:
        want_asm = (3 if c.get("per_traj") else 1) if herm else 2
    run.note(int(w["asm_kernel"]) == want_asm, f"asm_kernel {w['asm_kernel']}, expected {want_asm}")
    # few derivative batches: the workgroup-per-batch kernels (deriv_kernel<16/32>, deriv2_kernel), never a one-wave assembly kernel
    run.note(int(w["asm_deriv_kernel"]) == 0, f"asm_deriv_kernel {w['asm_deriv_kernel']} on the default route")
    # the scanned sweeps need N_T >= 64 (grape_create): none of these shapes has them
    run.note(int(w["scan_block"]) == 0, f"scan_block {w['scan_block']} at N_T = {c['N_T']}")
    if N >= 49 and herm:
        run.note(int(w["t16_cells"]) == c["K"] * c["N_T"], f"t16_cells {w['t16_cells']}")


# ------------------------------------------------------------------------------------------------------------ part A

def test_final_states_then_sums_between_two_replays(g, ref, monkeypatch):
    """between two replays of the captured evaluation, final_states() followed by sums() -- two copies
    that only read -- made the next grape_eval return GRAPE_ERR_AGAIN.  The shape is where it was seen (tools/hvp_ab.py, C2)."""
    pr = si.part_a_problem()
    run = Run(g, ref, monkeypatch, "partA", pr)
    with run.h as h:
        for i in range(4):                                       # uncaptured, uncaptured, capture + replay, replay
            run.check_eval(f"eval {i}", against_oracle=False, work=False)
        psiT = h.final_states()
        sums = h.sums()
        with run.twin() as t:
            t.eval(si.part_a_pulses(3))
            run.note(same(psiT, t.final_states()) and same(sums, t.sums()), "final_states / sums differ from the fresh handle's")
        x, _ = run.check_eval("eval after final_states, sums", against_oracle=True)
        w = h.work()
        # the statistics share the flag word's reset: what grape_get_work counts must be the fresh handle's as well
        with run.twin() as t:
            t.eval(x)
            wt = t.work()
        run.note(same(w, wt), f"work() after that eval differs from the fresh handle's: {differing(w, wt)}")
        run.note(int(w["scan_block"]) > 0, f"scan_block {w['scan_block']}: the scanned sweeps apply at N_T = 500")
        run.check_eval("the replay after it", against_oracle=False)
    run.report()


# ------------------------------------------------------------------------------------------------------------ part B

@pytest.mark.parametrize("cid", list(si.CASES))
def test_script_on_one_handle(g, ref, monkeypatch, cid):
    pr = si.problem(cid)
    c = si.CASES[cid]
    K, N, N_T, L = c["K"], c["N"], c["N_T"], c["L"]
    run = Run(g, ref, monkeypatch, cid, pr)
    frame_pr = dict(pr, shape=None)
    with run.h as h:
        # 1. four evaluations: uncaptured, uncaptured, capture + replay, replay
        for i in range(4):
            x, _ = run.check_eval(f"step 1, eval {i}", against_oracle=True if i == 2 else None, work=i == 3)
        kernels_asserted(run, h.work())

        # 2. every getter after a replay, then eval
        with run.twin() as t:
            t.eval(x)
            for name in si.GETTERS:
                a, b = run.getter(h, name), run.getter(t, name)
                run.note(same(a, b), f"step 2: {name}() differs from the fresh handle's" + (f": {differing(a, b)}" if name == "work" else ""))
        want = fr.evaluate(frame_pr, x, functional=c["f"])
        run.bar("dJdt vs frame reference", np.abs(h.time_gradient() - want["dJdt"]).max(), fr.tol_G(want["dJdt"]), "step 2")
        run.bar("tau_grads vs frame reference", np.abs(h.tau_grads() - want["tau_grads"]).max(), fr.tol_G(want["tau_grads"]), "step 2")
        run.bar("final_states vs frame reference", np.abs(h.final_states() - want["psiT"]).max(), 1e-12 * run.scale(want["tau"], want["psiT"]), "step 2")
        run.check_eval("step 2, eval after the getters", against_oracle=True)

        # 3. an evaluation without a gradient, then eval
        x = run.x()
        Jn, Gn, taun = h.eval(x, gradient=False)
        with run.twin() as t:
            run.note(same((Jn, Gn, taun), t.eval(x, gradient=False)), "step 3: eval(gradient=False) differs from the fresh handle's")
        if not run.heavy:
            Jr, _, taur, parts = run.oracle(x)
            run.bar("J vs oracle", abs(Jn - Jr), 1e-12 * run.scale(taur, parts["psiT"]), "step 3, no gradient")
        run.check_eval("step 3, eval after eval(gradient=False)")

        # 4. forward + final_states + backward_chi(chi), time_gradient, then eval
        x = run.x()
        tau = h.forward(x)
        psiT = h.final_states()
        chi = si.caller_chi(cid, psiT)
        Gc = h.backward_chi(chi)
        dJ = h.time_gradient()
        with run.twin() as t:
            tt = t.forward(x)
            pt = t.final_states()
            run.note(same((tau, psiT), (tt, pt)), "step 4: forward / final_states differ from the fresh handle's")
            run.note(same(Gc, t.backward_chi(chi)), "step 4: backward_chi differs from the fresh handle's")
            run.note(same(dJ, t.time_gradient()), "step 4: time_gradient after backward_chi differs from the fresh handle's")
        Gcr, _, psiTr, _ = ref.evaluate_chi(pr["H0"], pr["Hc"], pr["tlist"], x, pr["psi0"], pr["target"], chi, weights=pr["weights"])
        run.bar("psiT vs oracle", np.abs(psiT - psiTr).max(), 1e-12 * run.scale(tau, psiTr), "step 4")
        run.bar("G vs oracle", np.abs(Gc - Gcr).max(), 1e-10 * max(np.abs(Gcr).max(), 1e-3), "step 4, backward_chi")
        if not run.heavy:
            want = fr.evaluate(dict(frame_pr, chi=chi), x)
            run.bar("dJdt vs frame reference", np.abs(dJ - want["dJdt_prop"]).max(), fr.tol_G(want["dJdt_prop"]), "step 4, caller's chi")
        run.check_eval("step 4, eval after the split phases with chi")

        # 5. forward + sums + backward(f), then eval
        x = run.x()
        tau = h.forward(x)
        sm = h.sums()
        Gb = h.backward(complex(sm[0], sm[1]))
        with run.twin() as t:
            tt = t.forward(x)
            st = t.sums()
            run.note(same((tau, sm), (tt, st)), "step 5: forward / sums differ from the fresh handle's")
            run.note(same(Gb, t.backward(complex(st[0], st[1]))), "step 5: backward differs from the fresh handle's")
        if not run.heavy:
            Jr, Gr, taur, parts = run.oracle(x)
            run.bar("tau vs oracle", np.abs(tau - taur).max(), 1e-12 * run.scale(taur, parts["psiT"]), "step 5")
            run.bar("G vs oracle", np.abs(Gb - Gr).max(), 1e-10 * max(np.abs(Gr).max(), 1e-3), "step 5, backward")
        run.check_eval("step 5, eval after the split phases")

        # 7. hvp(V) with two directions after a replay, then eval
        x, _ = run.check_eval("step 7, eval before hvp")
        V = si.directions(cid, 2)
        Hv = h.hvp(V)
        with run.twin() as t:
            t.eval(x)
            run.note(same(Hv, t.hvp(V)), "step 7: hvp differs from the fresh handle's")
        if N <= HVP_REFERENCE_MAX_N:
            want = hr.evaluate(dict(frame_pr), x, V, c["f"])
            run.bar("Hv vs hvp reference", np.abs(Hv - want["Hv"]).max(), hr.tol_hv(want["Hv"]), "step 7")
        run.check_eval("step 7, eval after hvp")

        # 8. eval_batch with three pulse sets, then eval
        X = np.stack([run.x() for _ in range(3)])
        Jb, Gb, taub = h.eval_batch(X)
        route = h.batch_info()["route"]
        # the batched kernels exist for NP = 16 only; everything else is one ordinary evaluation per set, by the documented
        # envelope -- not a refusal, and on the single-wait path: three more calls towards the 16th
        print(cid, "eval_batch route", route)
        if cid == "s16h" or N > 16:
            run.note(route == (1 if N <= 16 else 0), f"step 8: route {route}")
        with run.twin() as t:
            run.note(same((Jb, Gb, taub), t.eval_batch(X)), "step 8: eval_batch differs from the fresh handle's")
        for p in range(1 if run.heavy else 3):
            Jr, Gr, taur, parts = run.oracle(X[p])
            sc = run.scale(taur, parts["psiT"])
            run.bar("J vs oracle", abs(Jb[p] - Jr), 1e-12 * sc, f"step 8, set {p}")
            run.bar("tau vs oracle", np.abs(taub[p] - taur).max(), 1e-12 * sc, f"step 8, set {p}")
            run.bar("G vs oracle", np.abs(Gb[p] - Gr).max(), 1e-10 * max(np.abs(Gr).max(), 1e-3), f"step 8, set {p}")
        run.check_eval("step 8, eval after eval_batch")

        # 9. sequential sweeps and back: the graph is captured again on each side
        x = run.x()
        h.set_fused_sweeps(False)
        got = h.eval(x)
        with run.twin() as t:
            t.set_fused_sweeps(False)
            run.note(same(got, t.eval(x)), "step 9: eval with sequential sweeps differs from the fresh handle's")
        if not run.heavy:
            Jr, Gr, taur, parts = run.oracle(x)
            run.bar("G vs oracle", np.abs(got[1] - Gr).max(), 1e-10 * max(np.abs(Gr).max(), 1e-3), "step 9, sequential sweeps")
        h.set_fused_sweeps(True)
        run.check_eval("step 9, eval with the concurrent sweeps again")

        # 10. across the 16th call of the single-wait path (uncaptured) and into the replays behind it
        for i in range(12):
            run.check_eval(f"step 10, eval {i}", against_oracle=i == 11, work=i == 11)
        kernels_asserted(run, h.work())

    # 6. the state running-cost family: a handle created with D, lambda_b; backward_xi between two replays
    rd = Run(g, ref, monkeypatch, cid, pr, with_D=True)
    with rd.h as h:
        for i in range(3):
            rd.check_eval(f"step 6, eval {i} with the built-in running cost", against_oracle=i == 2)
        x = rd.x()
        h.forward(x)
        fw = h.storage(0)
        xi = -np.einsum("ij,knj->kni", rd.D, fw)
        Gx = h.backward_xi(xi, si.LAMBDA_B)
        with rd.twin() as t:
            t.forward(x)
            run.note(same(fw, t.storage(0)), "step 6: storage(0) differs from the fresh handle's")
            run.note(same(Gx, t.backward_xi(xi, si.LAMBDA_B)), "step 6: backward_xi differs from the fresh handle's")
        Jr, Gr, taur, parts = rd.oracle(x)
        run.bar("G vs oracle", np.abs(Gx - Gr).max(), 1e-10 * max(np.abs(Gr).max(), 1e-3), "step 6, backward_xi")
        rd.check_eval("step 6, eval after backward_xi", against_oracle=False)
    run.bad += rd.bad
    for key, v in rd.worst.items():
        run.bar(key, v[0], v[1], v[2])
    run.report()


def test_every_ordered_pair_of_getters_between_two_replays(g, ref, monkeypatch):
    """the generalisation of part A: 81 pairs of getters on ONE handle, one replay after each pair"""
    cid = "s16h"
    pr = si.problem(cid)
    run = Run(g, ref, monkeypatch, cid, pr)
    xs = [si.pulses(cid, i) for i in range(4)]
    want, want_work = [], []
    with run.twin() as t:
        for x in xs:                                             # (a fresh handle per pulse would give the same bits: asserted above)
            want.append(t.eval(x))
            want_work.append(t.work())
    with run.h as h:
        n = 0
        for x, w in zip(xs, want):
            run.note(same(h.eval(x), w), f"eval {n}")
            n += 1
        for a in si.GETTERS:
            for b in si.GETTERS:
                run.getter(h, a)
                run.getter(h, b)
                x, w = xs[n % 4], want[n % 4]
                try:
                    run.note(same(h.eval(x), w), f"eval after {a}(), {b}() (call {n}) differs from the handle without a graph")
                    wh = h.work()
                    run.note(same(wh, want_work[n % 4]), f"work() after {a}(), {b}(), eval (call {n}): {differing(wh, want_work[n % 4])}")
                except g.GrapeHipError as e:
                    run.note(False, f"eval after {a}(), {b}() (call {n}) returned {e}")
                n += 1
    run.report()


def test_stale_state_sequence_across_set_tlist(g, ref, monkeypatch):
    """The sequence DESIGN.md 21 left out, back now that its cause is known: N = 64, cells at the edge of the
    four-product range; pulses A (cell X handed over), B (cell Y), A; set_tlist to a grid that moves X inside; an evaluation
    without a gradient; a capture with no cell handed over; storage / propagator / tau_grads / work between the replays; a
    replay with a cell handed over.  A reset of the flag word that a replay gets wrong starts the cell list counter
    (grape_t18.hip: cell_list[atomicAdd(&flags[4], 1)]) and the count of cells beyond the plan's range (flags[6]) from
    whatever it wrote.  Every step against a fresh handle without a graph, bit for bit, and the counts of the reference."""
    import t16_route_reference as R
    pr, A, B, grid2, X, Y = R.stale_problem()
    pr = dict(pr, N=64, N_T=len(pr["tlist"]) - 1, functional=0)
    run = Run(g, ref, monkeypatch, "stale", pr)

    def step(what, x, tlist, getters=(), oracle=False):
        run.pr = dict(pr, tlist=tlist)                           # (the twin is created on the grid the handle has now)
        for name in getters:
            run.getter(run.h, name)
        _, got = run.check_eval(what, x=x, against_oracle=oracle)
        dec = R.decide(R.with_pulses(dict(pr, shape=None), x, tlist))
        w = run.h.work()
        run.note(dec["counts"]["undecidable"] == 0, f"{what}: undecidable cell in the inputs")
        run.note(int(w["t16_cells"]) == dec["counts"]["t16_cells"], f"{what}: t16_cells {w['t16_cells']}, reference {dec['counts']['t16_cells']}")
        return dec["counts"]

    with run.h as h:
        t1 = pr["tlist"]
        cA = step("eval A", A, t1, oracle=True)
        cB = step("eval B", B, t1)
        step("eval A (capture and replay)", A, t1)
        run.note(cA["handed_over"] >= 1 and cB["handed_over"] >= 1, f"no cell handed over on the first grid: {cA}, {cB}")
        h.set_tlist(grid2)
        run.pr = dict(pr, tlist=grid2)
        Jn = h.eval(A, gradient=False)
        with run.twin() as t:
            run.note(same(Jn, t.eval(A, gradient=False)), "eval(gradient=False) after set_tlist differs from the fresh handle's")
        cA2 = step("eval A on the new grid (capture and replay)", A, grid2)
        cB2 = step("eval B on the new grid (replay, another cell handed over)", B, grid2,
                   getters=("propagator", "storage0", "storage1", "tau_grads", "work"), oracle=True)
        run.note(cA2["handed_over"] != cB2["handed_over"], f"the replay hands over what the capture did: {cA2}, {cB2}")
        step("eval A on the new grid (replay)", A, grid2, getters=("storage0", "sums", "final_states", "work"))
        step("eval B on the new grid (replay)", B, grid2)
    run.report()
