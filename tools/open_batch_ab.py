"""Open-system handles: what grape_open_eval_batch costs against one evaluation, and that the evaluation did not move against the
parent commit -- ONE process on one GPU.

  python tools/open_batch_ab.py [--old tools/_prev.so] [--d 16,32,64] [--K 1,8] [--P 0] [--J 2] [--steps 500] [--rounds 3]
                                [--reps 2] [--loop-sets 4]

Problem: synth.make_open_problem(d, L = 2, steps, K, J), dt = 1 (the shapes of tools/open_ab.py, tools/open_hvp_ab.py).  The pulse
sets are amplitude factors 0.5 ... 1.5 of the problem's pulse vector; P = 0 means P_max = 256 / (K L), one backward workgroup per
CU.  For every (d, K) and every round, in this order (old first, as the other A/B records of the project):
  eval_old   grape_eval with a gradient on the library of the PARENT commit (--old; left out without it); J and G are compared
             bit for bit with the current library's.  THE YARDSTICK of the batch figures.
  eval       the same on the current library -- must not move against eval_old by more than their run-to-run spread
  batch1     grape_open_eval_batch with P = 1
  batchP     grape_open_eval_batch with P sets: ms per call and per set
  loop       grape_eval_batch (one ordinary evaluation per set) -- timed on the first min(P, --loop-sets) sets and scaled to P:
             the loop is P independent evaluations by construction, and at d = 64 its full length is minutes per repetition
Each figure is ms (host wall time, minimum over --reps inside the round); the table prints the median over the rounds and the
spread (max - min).  Expectation: while K L P <= 256 a batch of P costs at most 1.25 x eval_old (the margin DESIGN.md 15 / 16 allow
for prologues and differing term counts); beyond, in proportion to ceil(K L P / 256)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from open_ab import open_handle_of, timed  # noqa: E402
from grape_jl_amd import api, synth  # noqa: E402

MARGIN = 1.25
L = 2
CUS = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit")
    ap.add_argument("--d", default="16,32,64")
    ap.add_argument("--K", default="1,8")
    ap.add_argument("--P", type=int, default=0, help="pulse sets (0: 256 / (K L))")
    ap.add_argument("--J", type=int, default=2)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--loop-sets", type=int, default=4)
    a = ap.parse_args()
    new = api.library_path()
    J = a.J
    rows = []
    for d in [int(x) for x in a.d.split(",") if x]:
        for K in [int(x) for x in a.K.split(",")]:
            P = a.P if a.P > 0 else max(1, CUS // (K * L))
            pr = synth.make_open_problem(d, L, a.steps, K, J, seed=synth.BASE_SEED ^ (1000 + d))
            x = pr["pulsevals"]
            X = np.ascontiguousarray(np.linspace(0.5, 1.5, P)[:, None] * x[None, :]) if P > 1 else x[None, :].copy()
            one = int(np.argmin(np.abs(np.linspace(0.5, 1.5, P) - 1.0))) if P > 1 else 0
            nloop = min(P, max(1, a.loop_sets))
            hs = {}
            if a.old:
                hs["eval_old"] = open_handle_of(a.old, pr)
            hs["eval"] = open_handle_of(new, pr)
            outs = {name: h.eval(x) for name, h in hs.items()}       # (warm-up, and the results to compare)
            hn = hs["eval"]
            bP = hn.open_eval_batch(X)                                       # (allocates the storage of the call)
            infoP = hn.open_batch_info()
            b1 = hn.open_eval_batch(X[one:one + 1])
            res = {name: [] for name in hs}
            res["batch1"], res["batchP"], res["loop"] = [], [], []
            reps = a.reps if d <= 32 else 1
            for _ in range(a.rounds if d <= 32 else max(2, a.rounds - 1)):
                for name, h in hs.items():
                    res[name].append(timed(lambda h=h: h.eval(x), reps))
                res["batch1"].append(timed(lambda: hn.open_eval_batch(X[one:one + 1]), reps))
                res["batchP"].append(timed(lambda: hn.open_eval_batch(X), reps))
                res["loop"].append(timed(lambda: hn.eval_batch(X[:nloop]), reps) * P / nloop)
            again = hn.open_eval_batch(X)
            Jn, Gn, taun = hn.eval(X[one])
            row = dict(d=d, K=K, J=J, steps=a.steps, P=P, rounds_ms=res, loop_sets_timed=nloop,
                       batch_repeats_bitwise=bool(all(np.array_equal(u, v) for u, v in zip(bP, again))),
                       set_independent_of_P=bool(all(np.array_equal(u[one], v[0]) for u, v in zip(bP, b1))),
                       batch_vs_eval=dict(dJ=float(abs(bP[0][one] - Jn)), dG_rel=float(np.abs(bP[1][one] - Gn).max() / np.abs(Gn).max()),
                                          dtau=float(np.abs(bP[2][one] - taun).max()),
                                          same_bits=bool(bP[0][one] == Jn and np.array_equal(bP[1][one], Gn) and np.array_equal(bP[2][one], taun))),
                       sets_per_group=infoP["sets_per_group"], groups=infoP["groups"], bytes=infoP["bytes"],
                       workgroups_backward=K * L * P)
            if a.old:
                Jo, Go, _ = outs["eval_old"]
                Jc, Gc, _ = outs["eval"]
                row["same_bits_as_old"] = bool(Jo == Jc and np.array_equal(Go, Gc))
            print(json.dumps(row), flush=True)
            rows.append(row)
            for h in hs.values():
                h.close()
    print("# medians over the rounds, ms (spread = max - min of the rounds); yardstick: eval_old (eval without --old)")
    print(f"# expectation: batchP <= {MARGIN} x ceil(K L P / {CUS}) x yardstick")
    print("# d K P | eval_old | eval | J, G same bits | batch P=1 | batch P | per set | loop of P (scaled from loop_sets_timed) | "
          "batch P / yardstick | allowed | within | loop / batch P")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        cell = lambda n: f"{med[n]:.2f} ({spr[n]:.2f})" if n in med else "-"   # noqa: E731
        yard = med.get("eval_old", med["eval"])
        allowed = MARGIN * -(-(r["K"] * L * r["P"]) // CUS)
        ratio = med["batchP"] / yard
        print(f"{r['d']} {r['K']} {r['P']} | {cell('eval_old')} | {cell('eval')} | {r.get('same_bits_as_old', '-')} | {cell('batch1')} | "
              f"{cell('batchP')} | {med['batchP'] / r['P']:.2f} | {cell('loop')} [{r['loop_sets_timed']}] | {ratio:.3f} | {allowed:.2f} | "
              f"{'yes' if ratio <= allowed else 'NO'} | {med['loop'] / med['batchP']:.1f}")


if __name__ == "__main__":
    main()
