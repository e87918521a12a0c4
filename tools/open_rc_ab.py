"""Open-system handles: what a state running cost (grape_open_set_running_cost) costs per evaluation with a gradient, and that
a handle WITHOUT a cost did not move against the parent commit -- ONE process on one GPU.

  python tools/open_rc_ab.py [--old tools/_prev.so] [--d 16,64] [--steps 500] [--rounds 3] [--reps 2]

Problem: synth.make_open_problem(d, L = 2, steps, K = 2, J = 2), dt = 1 (the shapes of tools/open_ab.py); D a random Hermitian
matrix of unit 2-norm, lambda_b = 0.25.  For every d and every round, in this order (old first, as the other A/B records of the
project):
  eval_old   grape_eval with a gradient on the library of the PARENT commit (--old; left out without it)
  plain      the same on the current library, on ONE handle whose cost has been removed (set_running_cost(None, 0)) -- must not
             move against eval_old by more than their run-to-run spread; J, G, tau and tau_grads are compared bit for bit with
             the parent's
  cost       the same handle with the cost set: lind_backward_rc_kernel, lind_gb_kernel and the J_b reduction
The handle alternates between plain and cost inside every round.  Each figure is ms (host wall time, minimum over --reps
inside the round); the table prints the median over the rounds and the spread (max - min), and the forward / backward launch
times of the handle (HIP events) with and without the cost."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from open_ab import open_handle_of, timed  # noqa: E402
from grape_jl_amd import api, synth  # noqa: E402

LAMBDA_B = 0.25


def outputs(h, x):
    J, G, tau = h.eval(x)
    return dict(J=J, G=G, tau=tau, tau_grads=h.tau_grads())


def same_bits(a, b):
    return bool(all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("J", "G", "tau", "tau_grads")))


def launch_ms(h, x):
    h.reset_timings()
    h.eval(x)
    t = h.timings()
    return t["forward"], t["backward"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit")
    ap.add_argument("--d", default="16,64")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    new = api.library_path()
    rows = []
    for d in [int(x) for x in a.d.split(",") if x]:
        pr = synth.make_open_problem(d, 2, a.steps, 2, 2, seed=synth.BASE_SEED ^ (1000 + d))
        x = pr["pulsevals"]
        D = synth.gue(synth.subseed(synth.BASE_SEED, 8200 + d), d)
        D = D / np.linalg.norm(D, 2)
        h_old = open_handle_of(a.old, pr) if a.old else None
        h = open_handle_of(new, pr)
        never = outputs(h, x)                                  # (a handle that never had a cost; warm-up)
        old = outputs(h_old, x) if h_old else None
        h.set_running_cost(D, LAMBDA_B)
        with_cost = outputs(h, x)
        Jb = float(h.sums()[4])
        h.set_running_cost(None, 0.0)
        removed = outputs(h, x)
        res = dict(eval_old=[], plain=[], cost=[])
        for _ in range(a.rounds):
            if h_old:
                res["eval_old"].append(timed(lambda: h_old.eval(x), a.reps))
            res["plain"].append(timed(lambda: h.eval(x), a.reps))
            h.set_running_cost(D, LAMBDA_B)
            res["cost"].append(timed(lambda: h.eval(x), a.reps))
            h.set_running_cost(None, 0.0)
        fwd_plain, bwd_plain = launch_ms(h, x)
        h.set_running_cost(D, LAMBDA_B)
        fwd_cost, bwd_cost = launch_ms(h, x)
        again = outputs(h, x)
        row = dict(d=d, K=2, L=2, J=2, steps=a.steps, lambda_b=LAMBDA_B, rounds_ms={k: v for k, v in res.items() if v},
                   forward_ms=dict(plain=fwd_plain, cost=fwd_cost), backward_ms=dict(plain=bwd_plain, cost=bwd_cost),
                   J_plain=never["J"], J_cost=with_cost["J"], J_b=Jb, dG_cost=float(np.abs(with_cost["G"] - never["G"]).max()),
                   removed_same_bits_as_never=same_bits(removed, never), cost_repeats_bitwise=same_bits(again, with_cost))
        if old:
            row["plain_same_bits_as_old"] = same_bits(never, old)
        print(json.dumps(row), flush=True)
        rows.append(row)
        for hh in (h, h_old):
            if hh:
                hh.close()
    print("# medians over the rounds, ms per evaluation with gradient (spread = max - min of the rounds); launches: HIP events")
    print("# d | eval_old | plain | J, G, tau, tau_grads same bits as old | cost | cost / plain | forward plain -> cost | backward plain -> cost")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        cell = lambda n: f"{med[n]:.2f} ({spr[n]:.2f})" if n in med else "-"   # noqa: E731
        print(f"{r['d']} | {cell('eval_old')} | {cell('plain')} | {r.get('plain_same_bits_as_old', '-')} | {cell('cost')} | "
              f"{med['cost'] / med['plain']:.3f} | {r['forward_ms']['plain']:.2f} -> {r['forward_ms']['cost']:.2f} | "
              f"{r['backward_ms']['plain']:.2f} -> {r['backward_ms']['cost']:.2f}")


if __name__ == "__main__":
    main()
