"""Open-system handles: what grape_open_time_gradient costs, and that the evaluation did not move against the parent commit --
ONE process on one GPU.

  python tools/open_tg_ab.py [--old tools/_prev.so] [--d 16,32,64] [--K 1,8] [--steps 500] [--rounds 3] [--reps 2]

Problem: synth.make_open_problem(d, L = 2, steps, K, J = 2), dt = 1 (the shapes of tools/open_ab.py).  For every (d, K) and every
round, in this order (old first, as the other A/B records of the project):
  eval_old   grape_eval with a gradient on the library of the PARENT commit (--old; left out without it); J and G are compared
             bit for bit with the current library's
  eval       the same on the current library -- must not move against eval_old by more than their run-to-run spread
  tg         grape_open_time_gradient after that evaluation: the ADDED host wall time of the call
Each figure is ms (host wall time, minimum over --reps inside the round); the table prints the median over the rounds and
the spread (max - min).  The yardstick of the cost is the forward launch of the same handle (timings()["forward"], HIP events):
the kernel executes the forward kernel's 2 + 2J products and two barriers per term over a chain of the same length, so the
condition is  tg <= 1.25 x forward  (the margin covers the different term counts of the adjoint chain, the prologue, the
reduction and the copy); the last column says whether it holds."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit")
    ap.add_argument("--d", default="16,32,64")
    ap.add_argument("--K", default="1,8")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    new = api.library_path()
    rows = []
    for d in [int(x) for x in a.d.split(",") if x]:
        for K in [int(x) for x in a.K.split(",")]:
            pr = synth.make_open_problem(d, 2, a.steps, K, 2, seed=synth.BASE_SEED ^ (1000 + d))
            x = pr["pulsevals"]
            hs = {}
            if a.old:
                hs["eval_old"] = open_handle_of(a.old, pr)
            hs["eval"] = open_handle_of(new, pr)
            outs = {name: h.eval(x) for name, h in hs.items()}       # (warm-up, and the results to compare)
            hn = hs["eval"]
            tg0 = hn.time_gradient()                                    # (allocates the buffers of the call)
            res = {name: [] for name in hs}
            res["tg"] = []
            reps = a.reps if d <= 32 else 1
            for _ in range(a.rounds if d <= 32 else max(2, a.rounds - 1)):
                for name, h in hs.items():
                    res[name].append(timed(lambda h=h: h.eval(x), reps))
                res["tg"].append(timed(hn.time_gradient, reps))
            hn.reset_timings()
            Jn, Gn, _ = hn.eval(x)
            t = hn.timings()
            tg1 = hn.time_gradient()
            t_after = hn.timings()
            row = dict(d=d, K=K, steps=a.steps, rounds_ms=res, forward_ms=t["forward"], backward_ms=t["backward"],
                       timings_untouched=t == t_after, tg_repeats_bitwise=bool(np.array_equal(tg0, tg1)),
                       tg_max=float(np.abs(tg1).max()))
            if a.old:
                Jo, Go, _ = outs["eval_old"]
                row["same_bits_as_old"] = bool(Jo == Jn and np.array_equal(Go, Gn))
            print(json.dumps(row), flush=True)
            rows.append(row)
            for h in hs.values():
                h.close()
    print("# medians over the rounds, ms (spread = max - min of the rounds); forward: the forward launch of the same handle (HIP events)")
    print(f"# d K | eval_old | eval | J, G same bits | tg (added) | forward launch | tg / forward | <= {MARGIN}")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        cell = lambda n: f"{med[n]:.2f} ({spr[n]:.2f})" if n in med else "-"   # noqa: E731
        ratio = med["tg"] / r["forward_ms"]
        print(f"{r['d']} {r['K']} | {cell('eval_old')} | {cell('eval')} | {r.get('same_bits_as_old', '-')} | {cell('tg')} | "
              f"{r['forward_ms']:.2f} | {ratio:.3f} | {'yes' if ratio <= MARGIN else 'NO'}")


if __name__ == "__main__":
    main()
