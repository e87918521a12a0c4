"""A/B timing of the time gradient (ABI v7) at a BASELINE shape, in one process, alternating:

  eval        grape_eval with a gradient
  eval+tg     grape_eval followed by grape_get_time_gradient
  pseudo      the pseudo-control route it replaces: drift as an extra control per trajectory (H0' = 0), grape_eval
  set_tlist   grape_set_tlist (then one evaluation is NOT included)
  create      a fresh grape_create of the same problem (what changing T cost before)

Prints one JSON line of medians in ms.  Usage: python tools/time_grid_ab.py [C3] [--reps 10] [--K 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import grape_jl_amd as g  # noqa: E402
from grape_jl_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C3")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--K", type=int, default=None, help="trajectories (default: the configuration's; C5 shard: 8)")
    a = ap.parse_args()
    pr = synth.make_config(a.config, K=a.K)
    K, N_T = pr["K"], pr["N_T"]
    args = (pr["H0"], pr["Hc"], pr["tlist"], pr["psi0"], pr["target"])
    x = pr["pulsevals"]
    Hp = np.concatenate([pr["H0"][:, None], np.broadcast_to(pr["Hc"], (K,) + pr["Hc"].shape)], axis=1)
    xp = np.concatenate([np.ones(N_T), x])
    t2 = pr["tlist"] * 1.01
    h = g.GrapeHip(*args)
    hp = g.GrapeHip(np.zeros_like(pr["H0"]), Hp, pr["tlist"], pr["psi0"], pr["target"])
    for _ in range(3):
        h.eval(x)
        h.time_gradient()
        hp.eval(xp)
    res = {k: [] for k in ("eval", "eval+tg", "tg", "pseudo", "set_tlist", "create")}
    for r in range(a.reps):
        t0 = time.perf_counter()
        h.eval(x)
        t1 = time.perf_counter()
        h.eval(x)
        t2_ = time.perf_counter()
        h.time_gradient()
        t3 = time.perf_counter()
        hp.eval(xp)
        t4 = time.perf_counter()
        h.set_tlist(t2 if r % 2 == 0 else pr["tlist"])
        t5 = time.perf_counter()
        if r < 3:   # (a create costs seconds at the larger shapes)
            hc = g.GrapeHip(*args)
            t6 = time.perf_counter()
            hc.close()
            res["create"].append((t6 - t5) * 1e3)
        res["eval"].append((t1 - t0) * 1e3)
        res["eval+tg"].append((t3 - t1) * 1e3)
        res["tg"].append((t3 - t2_) * 1e3)
        res["pseudo"].append((t4 - t3) * 1e3)
        res["set_tlist"].append((t5 - t4) * 1e3)
    h.close()
    hp.close()
    out = {"config": a.config, "K": K, "N": pr["N"], "L": pr["L"], "N_T": N_T, "reps": a.reps}
    out.update({k + "_ms": float(np.median(v)) for k, v in res.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
