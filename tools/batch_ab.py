"""A/B timing of grape_eval_batch: P pulse vectors in one call against P ordinary evaluations, in ONE process on one GPU.

  python tools/batch_ab.py [--old tools/_prev.so] [--cases C1:1,C2:1,C2:4,C2:32] [--P 16,64] [--rounds 3] [--reps 5]

For every (shape, K, P) and every round, in this order (old first, as the other A/B records of the project):
  old_loop    P grape_eval calls with fresh pulses on a handle of the OLD library (--old: a build of the parent commit, kept
              as tools/_prev.so; left out without it)
  new_loop    the same P calls on a handle of the current library
  batch_loop  eval_batch on a handle created under GRAPE_BATCH=0 (one ordinary evaluation per set inside the library)
  batch       eval_batch on a handle created under GRAPE_BATCH=1 (the batched kernels)
  batch_rule  eval_batch on a handle created without the variable (the route rule decides; the route is printed)
Each figure is the host wall time of the P evaluations in ms, the minimum over --reps repetitions inside the round.  Prints one
JSON line per case with the per-round figures, then a table of medians."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_lib import handle_of  # noqa: E402
from grape_jl_amd import api, synth  # noqa: E402


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit (baseline)")
    ap.add_argument("--cases", default="C1:1,C2:1,C2:4,C2:32")
    ap.add_argument("--P", default="16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    new = api.library_path()
    rows = []
    for case in a.cases.split(","):
        cid, K = case.split(":")
        pr = synth.make_config(cid, K=int(K))   # (C1, the README two-level problem, has one trajectory whatever K says)
        LN = pr["L"] * pr["N_T"]
        hs = {}
        if a.old:
            hs["old_loop"] = handle_of(a.old, pr)
        hs["new_loop"] = handle_of(new, pr)
        hs["batch_loop"] = handle_of(new, pr, {"GRAPE_BATCH": 0})
        hs["batch"] = handle_of(new, pr, {"GRAPE_BATCH": 1})
        hs["batch_rule"] = handle_of(new, pr)
        for P in [int(x) for x in a.P.split(",")]:
            u = 2.0 * synth.uniform01(1234 + P, P * LN).reshape(P, LN) - 1.0
            X = pr["pulsevals"][None, :] + 0.05 * u
            run = {}
            for name, h in hs.items():
                if name.endswith("_loop") and not name.startswith("batch"):
                    run[name] = (lambda h=h: [h.eval(X[p]) for p in range(P)])
                else:
                    run[name] = (lambda h=h: h.eval_batch(X))
            for fn in run.values():   # warm-up: module loads, batch storage, the captured graph of the ordinary path
                fn()
                fn()
            res = {name: [] for name in run}
            for _ in range(a.rounds):
                for name, fn in run.items():
                    res[name].append(timed(fn, a.reps))
            Jb, Gb, _ = hs["batch"].eval_batch(X)
            ref = [hs["new_loop"].eval(X[p]) for p in range(P)]
            dJ = max(abs(Jb[p] - ref[p][0]) for p in range(P))
            dG = max(np.abs(Gb[p] - ref[p][1]).max() for p in range(P))
            hs["batch_rule"].eval_batch(X)
            row = dict(shape=cid, N=pr["N"], L=pr["L"], N_T=pr["N_T"], K=pr["K"], P=P, rounds_ms=res, dJ=dJ, dG=dG,
                       rule_route=hs["batch_rule"].batch_info()["route"], info=hs["batch"].batch_info())
            print(json.dumps(row), flush=True)
            rows.append(row)
        for h in hs.values():
            h.close()
    names = [n for n in ("old_loop", "new_loop", "batch_loop", "batch", "batch_rule") if n in rows[0]["rounds_ms"]]
    print("# medians over the rounds, ms for P evaluations (spread = max - min of the rounds)")
    print("# shape K P | " + " | ".join(names) + " | rule route | old_loop / batch")
    for r in rows:
        med = {n: float(np.median(r["rounds_ms"][n])) for n in names}
        spr = {n: max(r["rounds_ms"][n]) - min(r["rounds_ms"][n]) for n in names}
        base = med.get("old_loop", med["new_loop"])
        print(f"{r['shape']} {r['K']} {r['P']} | " + " | ".join(f"{med[n]:.3f} ({spr[n]:.3f})" for n in names) +
              f" | {r['rule_route']} | {base / med['batch']:.1f}x")


if __name__ == "__main__":
    main()
