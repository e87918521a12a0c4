"""Timing of grape_hessian next to the route through grape_hvp with unit directions, and grape_eval around it, in ONE process.

  python tools/hessian_ab.py [--cases C2,N32,C3] [--rounds 3] [--reps 2] [--block 64] [--out profiles/hessian_ab.txt]

Shapes: C2 and C3 of synth.CONFIGS, and N32 = (N, L, N_T, K) = (32, 2, 200, 8).  For every shape and every round:
  eval       ms per grape_eval with a gradient
  hessian    ms of one grape_hessian (host wall time of the call, the copy of the matrix included)
  hvp_ident  ms of the Hessian through grape_hvp: the unit directions e_q in one call (existing code, not changed by
             grape_hessian).  Beyond --block * 8 directions a block of --block unit directions, taken from the middle of the
             pulse, is timed and scaled by L*N_T / block; the row says `scaled`.
Each figure is the minimum over --reps repetitions inside the round; the table gives the median of the rounds and their spread
(max - min).  ratio = hvp_ident / hessian.  The three term counters of grape_get_hessian_info follow, then whether J and G of a
grape_eval after the calls are bit for bit those before (eval_bitwise), and the largest deviation of the matrix from the
timed grape_hvp columns relative to ||H||_inf (dev_vs_hvp).  A shape whose Hessian storage the device cannot hold is left out,
and the output says so."""
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

EXTRA = {"N32": (32, 2, 200, 8)}


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="C2,N32,C3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--block", type=int, default=64)
    ap.add_argument("--out", default=None, help="also write the output to this file")
    a = ap.parse_args()
    lines = ["# python tools/hessian_ab.py " + " ".join(sys.argv[1:])]

    def say(text):
        print(text, flush=True)
        lines.append(text)

    path = api.library_path()
    rows = []
    for cid in a.cases.split(","):
        N, L, N_T, K = EXTRA.get(cid) or synth.CONFIGS[cid]
        tag = int("".join(ch for ch in cid if ch.isdigit()))
        pr = synth.make_problem(N, L, N_T, K, seed=synth.BASE_SEED ^ tag)
        P, x = L * N_T, pr["pulsevals"]
        h = handle_of(path, pr)
        J0, G0, _ = h.eval(x)
        try:
            H = h.hessian()
        except api.GrapeHipError as exc:
            say(f"# {cid}: left out, the Hessian storage does not fit: {exc}")
            h.close()
            continue
        scaled = P > 8 * a.block
        cols = np.arange(P) if not scaled else (P // 2 - a.block // 2 + np.arange(a.block))
        V = np.zeros((len(cols), P))
        V[np.arange(len(cols)), cols] = 1.0
        Hv = h.hvp(V)                                    # (warm-up of the HVP storage as well)
        dev = float(np.abs(H[cols] - Hv).max() / np.abs(H).max())
        res = {"eval": [], "hessian": [], "hvp_ident": []}
        for _ in range(a.rounds):
            res["eval"].append(timed(lambda: h.eval(x), a.reps))
            res["hessian"].append(timed(h.hessian, a.reps))
            res["hvp_ident"].append(timed(lambda: h.hvp(V), a.reps) * P / len(cols))
        info = h.hessian_info()
        J1, G1, _ = h.eval(x)
        row = dict(shape=cid, N=N, L=L, N_T=N_T, K=K, rounds_ms=res, scaled=bool(scaled), hvp_directions_timed=len(cols), info=info,
                   eval_bitwise=bool(J0 == J1 and np.array_equal(G0, G1)), dev_vs_hvp=dev,
                   symmetric=bool(np.array_equal(H, H.T)))
        say(json.dumps(row))
        rows.append(row)
        h.close()
    say("# medians over the rounds in ms (spread = max - min of the rounds)")
    say("# shape N L N_T K | eval | hessian | hvp_ident | ratio | terms forward seeds / backward seeds / fan | traj per pass | MB held | eval bitwise | dev vs hvp")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        i = r["info"]
        say(f"{r['shape']} {r['N']} {r['L']} {r['N_T']} {r['K']} | " + " | ".join(f"{med[n]:.3f} ({spr[n]:.3f})" for n in ("eval", "hessian")) +
            f" | {med['hvp_ident']:.1f} ({spr['hvp_ident']:.1f}){' scaled from ' + str(r['hvp_directions_timed']) + ' directions' if r['scaled'] else ''}"
            f" | {med['hvp_ident'] / med['hessian']:.1f} | {i['terms_forward_seeds']} / {i['terms_backward_seeds']} / {i['terms_fan']}"
            f" | {i['traj_per_pass']} | {i['bytes'] / 2 ** 20:.0f} | {r['eval_bitwise']} | {r['dev_vs_hvp']:.1e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
