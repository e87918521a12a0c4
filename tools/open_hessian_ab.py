"""Timing of grape_open_hessian next to the route through grape_open_hvp with unit directions, and the evaluation around it
against the parent commit's library, in ONE process, one handle per shape.

  python tools/open_hessian_ab.py [--shapes 16:1:2:100:8,32:2:2:100:8,64:2:2:50:4] [--old tools/_prev.so] [--rounds 3] [--reps 2]
                                  [--out profiles/open_hessian_ab.txt]

A shape is d:J:L:N_T:K of synth.make_open_problem (dt = 1).  For every shape and every round:
  eval_old   ms per grape_eval with a gradient on the library of the PARENT commit (--old; left out without it); J and G are
             compared bit for bit with the current library's
  eval       the same on the current library
  hessian    ms of one grape_open_hessian (host wall time of the call, the copy of the matrix included)
  hvp_ident  ms of the Hessian through grape_open_hvp: all L*N_T unit directions in one call (the parent's code, unchanged)
Each figure is the minimum over --reps repetitions inside the round; the table gives the median of the rounds and their spread
(max - min).  ratio = hvp_ident / hessian; `beats` says whether hvp_ident - hessian exceeds the spread of hvp_ident.  The
series terms per kernel of grape_get_open_hessian_info follow, the MB the call holds, whether J and G of a grape_eval after
the calls are bit for bit those before (eval_bitwise), and the largest deviation of the matrix from the grape_open_hvp columns
relative to ||H||_inf (dev_vs_hvp)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from open_ab import open_handle_of, timed  # noqa: E402
from grape_jl_amd import api, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16:1:2:100:8,32:2:2:100:8,64:2:2:50:4")
    ap.add_argument("--old", default=None, help="library built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the output to this file")
    a = ap.parse_args()
    lines = ["# python tools/open_hessian_ab.py " + " ".join(sys.argv[1:])]

    def say(text):
        print(text, flush=True)
        lines.append(text)

    new = api.library_path()
    rows = []
    for spec in a.shapes.split(","):
        d, J, L, N_T, K = (int(v) for v in spec.split(":"))
        pr = synth.make_open_problem(d, L, N_T, K, J, seed=synth.BASE_SEED ^ (1000 + d))
        P, x = L * N_T, pr["pulsevals"]
        hs = {}
        if a.old:
            hs["eval_old"] = open_handle_of(a.old, pr)
        hs["eval"] = open_handle_of(new, pr)
        outs = {name: h.eval(x) for name, h in hs.items()}       # (warm-up, and the results to compare)
        h = hs["eval"]
        J0, G0, _ = outs["eval"]
        H = h.open_hessian()                                     # (allocates the storage of the call)
        E = np.eye(P)
        Hv = h.open_hvp(E)                                       # (... and that of the unit-direction route)
        dev = float(np.abs(H - Hv).max() / np.abs(H).max())
        res = {name: [] for name in hs}
        res["hessian"], res["hvp_ident"] = [], []
        for _ in range(a.rounds):
            for name, hh in hs.items():
                res[name].append(timed(lambda hh=hh: hh.eval(x), a.reps))
            res["hessian"].append(timed(h.open_hessian, a.reps))
            res["hvp_ident"].append(timed(lambda: h.open_hvp(E), a.reps))
        info, hvinfo = h.open_hessian_info(), h.open_hvp_info()
        J1, G1, _ = h.eval(x)
        row = dict(shape=spec, d=d, J=J, L=L, N_T=N_T, K=K, rounds_ms=res, info=info, hvp_info=hvinfo,
                   eval_bitwise=bool(J0 == J1 and np.array_equal(G0, G1)), dev_vs_hvp=dev, symmetric=bool(np.array_equal(H, H.T)))
        if a.old:
            Jo, Go, _ = outs["eval_old"]
            row["dJ_old"], row["dG_old"] = float(abs(Jo - J0)), float(np.abs(Go - G0).max())
        say(json.dumps(row))
        rows.append(row)
        for hh in hs.values():
            hh.close()
    say("# medians over the rounds in ms (spread = max - min of the rounds)")
    say("# shape d:J:L:N_T:K | eval_old | eval | dJ dG against old | hessian | hvp_ident | ratio | beats by more than the spread | "
        "terms forward seeds / backward seeds / fan | hvp terms | traj per pass | MB held (hessian / hvp) | eval bitwise | dev vs hvp")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        i = r["info"]
        fig = lambda n: f"{med[n]:.3f} ({spr[n]:.3f})" if n in med else "-"   # noqa: E731
        say(f"{r['shape']} | {fig('eval_old')} | {fig('eval')} | {r.get('dJ_old', '-')} {r.get('dG_old', '-')} | {fig('hessian')} | {fig('hvp_ident')}"
            f" | {med['hvp_ident'] / med['hessian']:.1f} | {med['hvp_ident'] - med['hessian'] > spr['hvp_ident']}"
            f" | {i['terms_forward_seeds']} / {i['terms_backward_seeds']} / {i['terms_fan']} | {r['hvp_info']['series_terms']}"
            f" | {i['traj_per_pass']} | {i['bytes'] / 2 ** 20:.0f} / {r['hvp_info']['bytes'] / 2 ** 20:.0f} | {r['eval_bitwise']} | {r['dev_vs_hvp']:.1e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
