"""Open-system handles: what grape_open_hvp costs per direction, and that the evaluation did not move against the parent commit --
ONE process on one GPU.

  python tools/open_hvp_ab.py [--old tools/_prev.so] [--d 16,32,64] [--K 1,8] [--J 2] [--steps 500] [--rounds 3] [--reps 2] [--split]

Problem: synth.make_open_problem(d, L = 2, steps, K, J), dt = 1 (the shapes of tools/open_ab.py, tools/open_tg_ab.py).  For every
(d, K) and every round, in this order (old first, as the other A/B records of the project):
  eval_old   grape_eval with a gradient on the library of the PARENT commit (--old; left out without it); J and G are compared
             bit for bit with the current library's
  eval       the same on the current library -- must not move against eval_old by more than their run-to-run spread
  hvp1       grape_open_hvp with nv = 1 after that evaluation
  hvp16      grape_open_hvp with nv = 16: ms per call and per direction
Each figure is ms (host wall time, minimum over --reps inside the round); the table prints the median over the rounds and the
spread (max - min).  The yardstick of the cost comes from the product counts, not from the new kernels: a tangent forward term is
6 + 4J products against the 2 + 2J of the forward launch, a backward term 16 + 8J against the 6 + 4J of the backward launch, over
chains of the same length, so a direction should cost at most
    1.25 x [ (6 + 4J) / (2 + 2J) x forward + (16 + 8J) / (6 + 4J) x backward ]
with forward / backward the launch times of the same handle (timings(), HIP events); the 1.25 is the margin DESIGN.md 15 allowed for
differing term counts and prologues.  nv = 16 should cost about what nv = 1 does while K L nv <= 256 workgroups (one per CU).

--split adds, alternating with them inside every round, for nv = 1, 4, 16:
  hvp_old<nv>  grape_open_hvp on the library of the parent commit (--old), compared bit for bit with the current library's
  hvp<nv>      grape_open_hvp (nv = 4 is added)
  split<nv>    grape_open_hvp_forward + grape_open_hvp_backward(f, dsums) of the same directions: the same sweep kernels, two
               one-wave kernels and one more synchronisation; split_bitwise: the halves give the bits of grape_open_hvp
  chi<nv>      grape_open_hvp_forward with rho'(T) copied out + grape_open_hvp_backward_chi with chi = c sigma, chi' = c' sigma
               formed in numpy from tau, tau' (the same series through the restated kernel, one upload); chi_rel: its deviation
               from grape_open_hvp relative to ||Hv||_inf
A second table prints them, ms per call."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit")
    ap.add_argument("--d", default="16,32,64")
    ap.add_argument("--K", default="1,8")
    ap.add_argument("--J", type=int, default=2)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--split", action="store_true", help="time the split-phase calls next to grape_open_hvp")
    a = ap.parse_args()
    new = api.library_path()
    J = a.J
    rows = []
    for d in [int(x) for x in a.d.split(",") if x]:
        for K in [int(x) for x in a.K.split(",")]:
            pr = synth.make_open_problem(d, L, a.steps, K, J, seed=synth.BASE_SEED ^ (1000 + d))
            x = pr["pulsevals"]
            V = 2.0 * synth.uniform01(synth.subseed(d, 9100), 16 * x.size).reshape(16, x.size) - 1.0
            hs = {}
            if a.old:
                hs["eval_old"] = open_handle_of(a.old, pr)
            hs["eval"] = open_handle_of(new, pr)
            outs = {name: h.eval(x) for name, h in hs.items()}       # (warm-up, and the results to compare)
            hn = hs["eval"]
            hv16 = hn.open_hvp(V)                                            # (allocates the storage of the call)
            hv1 = hn.open_hvp(V[0])
            res = {name: [] for name in hs}
            res["hvp1"], res["hvp16"] = [], []
            reps = a.reps if d <= 32 else 1
            extra, split_fig = {}, {}
            if a.split:
                extra, split_fig = split_variants(hs, hn, pr, V, K)
                res.update({name: [] for name in extra})
            for _ in range(a.rounds if d <= 32 else max(2, a.rounds - 1)):
                for name, h in hs.items():
                    res[name].append(timed(lambda h=h: h.eval(x), reps))
                res["hvp1"].append(timed(lambda: hn.open_hvp(V[0]), reps))
                res["hvp16"].append(timed(lambda: hn.open_hvp(V), reps))
                for name, fn in extra.items():
                    res[name].append(timed(fn, reps))
            info16 = hn.open_hvp_info()
            hn.reset_timings()
            Jn, Gn, _ = hn.eval(x)
            t = hn.timings()
            again = hn.open_hvp(V)
            t_after = hn.timings()
            row = dict(d=d, K=K, J=J, steps=a.steps, rounds_ms=res, forward_ms=t["forward"], backward_ms=t["backward"],
                       timings_untouched=t == t_after, hvp_repeats_bitwise=bool(np.array_equal(hv16, again)),
                       direction_independent_of_nv=bool(np.array_equal(hv16[0], hv1)), hv_max=float(np.abs(hv16).max()),
                       dirs_per_group=info16["dirs_per_group"], bytes=info16["bytes"], workgroups_backward=K * L * 16, **split_fig)
            if a.old:
                Jo, Go, _ = outs["eval_old"]
                row["same_bits_as_old"] = bool(Jo == Jn and np.array_equal(Go, Gn))
            print(json.dumps(row), flush=True)
            rows.append(row)
            for h in hs.values():
                h.close()
    print("# medians over the rounds, ms (spread = max - min of the rounds); forward / backward: the launches of the same handle (HIP events)")
    print(f"# yardstick = {MARGIN} x [(6+4J)/(2+2J) forward + (16+8J)/(6+4J) backward]")
    print("# d K | eval_old | eval | J, G same bits | hvp nv=1 | hvp nv=16 | per direction at 16 | forward | backward | yardstick | "
          "nv=1 / yardstick | within | nv=16 / nv=1")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        cell = lambda n: f"{med[n]:.2f} ({spr[n]:.2f})" if n in med else "-"   # noqa: E731
        J = r["J"]
        yard = MARGIN * ((6 + 4 * J) / (2 + 2 * J) * r["forward_ms"] + (16 + 8 * J) / (6 + 4 * J) * r["backward_ms"])
        ratio = med["hvp1"] / yard
        print(f"{r['d']} {r['K']} | {cell('eval_old')} | {cell('eval')} | {r.get('same_bits_as_old', '-')} | {cell('hvp1')} | {cell('hvp16')} | "
              f"{med['hvp16'] / 16:.2f} | {r['forward_ms']:.2f} | {r['backward_ms']:.2f} | {yard:.2f} | {ratio:.3f} | "
              f"{'yes' if ratio <= 1.0 else 'NO'} | {med['hvp16'] / med['hvp1']:.2f}")
    if a.split:
        print("# --split: ms per call, median over the rounds (spread); old = grape_open_hvp of the parent's library")
        print("# d K nv | hvp_old | hvp | split | chi | split / hvp | chi / hvp | hvp same bits as old | split bitwise | chi rel")
        for r in rows:
            med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
            spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
            cell = lambda n: f"{med[n]:.2f} ({spr[n]:.2f})" if n in med else "-"   # noqa: E731
            for nv in SPLIT_NV:
                print(f"{r['d']} {r['K']} {nv} | {cell(f'hvp_old{nv}')} | {cell(f'hvp{nv}')} | {cell(f'split{nv}')} | {cell(f'chi{nv}')} | "
                      f"{med[f'split{nv}'] / med[f'hvp{nv}']:.4f} | {med[f'chi{nv}'] / med[f'hvp{nv}']:.4f} | {r.get('hvp_same_bits_as_old', '-')} | "
                      f"{r['split_bitwise']} | {r['chi_rel']:.1e}")


SPLIT_NV = (1, 4, 16)


def split_variants(hs, hn, pr, V, K):
    """the timed calls of --split (name -> callable) and their correctness figures, after the warm-up that allocates their storage"""
    sg, w = pr["target"], np.ones(K) if pr["weights"] is None else np.asarray(pr["weights"])
    f = complex(*hn.sums()[:2])
    whole = hn.open_hvp(V)

    def split(nv):
        _, dsums = hn.open_hvp_forward(V[:nv])
        return hn.open_hvp_backward(f, dsums)

    def chi(nv):
        _, dsums, _ = hn.open_hvp_forward(V[:nv], final_states=True)
        c, dc = w * f / K ** 2, w[None] * dsums[:, None] / K ** 2          # J_T_sm, the functional of open_handle_of
        return hn.open_hvp_backward_chi(c[:, None, None] * sg, dc[:, :, None, None] * sg[None])

    fig = dict(split_bitwise=bool(np.array_equal(split(16), whole)),
               chi_rel=float(np.abs(chi(16) - whole).max() / np.abs(whole).max()))
    if "eval_old" in hs:
        fig["hvp_same_bits_as_old"] = bool(np.array_equal(hs["eval_old"].open_hvp(V), whole))
    run = {}
    for nv in SPLIT_NV:
        if "eval_old" in hs:
            run[f"hvp_old{nv}"] = lambda nv=nv: hs["eval_old"].open_hvp(V[:nv])
        if nv not in (1, 16):
            run[f"hvp{nv}"] = lambda nv=nv: hn.open_hvp(V[:nv])
        run[f"split{nv}"] = lambda nv=nv: split(nv)
        run[f"chi{nv}"] = lambda nv=nv: chi(nv)
    return run, fig


if __name__ == "__main__":
    main()
