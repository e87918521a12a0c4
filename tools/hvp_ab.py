"""Timing of grape_hvp next to grape_eval, and the A/B of grape_eval against a build of the parent commit, in ONE process.

  python tools/hvp_ab.py [--old tools/_prev.so] [--cases C2,C3,X32] [--K k] [--steps n] [--nv 1,16] [--rounds 3] [--reps 3] [--split]

For every shape and every round, in this order (old first, as the other A/B records of the project):
  old_eval   ms per grape_eval with a gradient on a handle of the OLD library (--old: a build of the parent commit, kept as
             tools/_prev.so; left out without it)
  new_eval   the same on a handle of the current library -- the one condition on time: within the run-to-run spread of
             old_eval, and J and G bit for bit the old library's (printed as eval_bitwise)
  hvp_<nv>   ms PER DIRECTION of one grape_hvp call with nv directions (host wall time of the call / nv)
  --split adds, alternating with them in the same rounds:
  split_<nv> grape_hvp_forward + grape_hvp_backward(f, dsums) of the same directions, per direction
  chi_<nv>   grape_hvp_forward (with Psi'(T) copied out) + grape_hvp_backward_chi, per direction; chi = c_k tgt_k and
             chi' = c'_k tgt_k of the built-in functional, formed in numpy beforehand (outside the timing), so that the series
             are the ones grape_hvp runs.  split_bitwise: the halves give the bits of grape_hvp; chi_rel: the caller's route
             against it, relative to ||Hv||_inf.
With --old, hvp_bitwise: grape_hvp of the current library gives the bits of the old library's (where the old one has it).
Each figure is the minimum over --reps repetitions inside the round; the table gives the median of the rounds and their spread
(max - min).  mfma_frac: the flop of the matrix instructions the two sweeps of the nv = max call EXECUTED per second of the
call, as a fraction of the peak of the CUs the launch occupies (78.6 TF/s / 256 per CU, K nv workgroups, at most 256 CUs) --
counted from the series terms grape_get_hvp_info reports: per term and workgroup NP / 16 waves x NP / 4 slices x 4 real
products x 2048 flop for every operator product of the block recursion (forward: A, B; backward: A^+, B^+ and one per control
and column tile that holds its p or p' column).  --K / --steps shrink a shape (the serial length of a direction is N_T steps)."""
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

PEAK_PER_CU = 78.6e12 / 256


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def mfma_flop(info, N, L):
    """flop of the matrix instructions behind the series terms of one grape_hvp call"""
    NP = 16 * ((N + 15) // 16)
    per_product = (NP // 16) * (NP // 4) * 4 * 2048
    tiles = 2 if 2 + 2 * L > 16 else 1
    d_products = sum(len({(2 + l) // 16, (2 + L + l) // 16}) for l in range(L))
    return per_product * (2 * info["terms_forward"] + (2 * tiles + d_products) * info["terms_backward"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit (baseline of grape_eval)")
    ap.add_argument("--cases", default="C2,C3,X32")
    ap.add_argument("--K", type=int, default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--nv", default="1,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--split", action="store_true", help="time the split-phase calls next to grape_hvp")
    a = ap.parse_args()
    nvs = [int(x) for x in a.nv.split(",")]
    new_path = api.library_path()   # (before handle_of points the binding at another library)
    rows = []
    for cid in a.cases.split(","):
        N, L, N_T, K = synth.CONFIGS[cid]
        tag = int("".join(ch for ch in cid if ch.isdigit()))
        pr = synth.make_problem(N, L, a.steps or N_T, a.K or K, seed=synth.BASE_SEED ^ tag)
        LN = pr["L"] * pr["N_T"]
        x = pr["pulsevals"]
        V = 2.0 * synth.uniform01(77, max(nvs) * LN).reshape(max(nvs), LN) - 1.0
        hs = {}
        if a.old:
            hs["old_eval"] = handle_of(a.old, pr)
        hs["new_eval"] = handle_of(new_path, pr)
        h = hs["new_eval"]
        run = {name: (lambda hh=hh: hh.eval(x)) for name, hh in hs.items()}
        for nv in nvs:
            run[f"hvp_{nv}"] = (lambda nv=nv: h.hvp(V[:nv]))
        split_bitwise = chi_rel = None
        if a.split:
            K, w = pr["K"], pr["weights"]
            _, _, tau = h.eval(x)
            f_total = complex(*h.sums()[:2])
            dtau, dsums = h.hvp_forward(V)
            chi = (w * np.sum(w * tau) / K ** 2)[:, None] * pr["target"]                   # J_T_sm (include/grape_hip.h)
            dchi = (w[None, :] * np.sum(w[None, :] * dtau, axis=1)[:, None] / K ** 2)[:, :, None] * pr["target"][None]
            whole = h.hvp(V)
            h.hvp_forward(V)
            split_bitwise = bool(np.array_equal(h.hvp_backward(f_total, dsums), whole))
            chi_rel = float(np.abs(h.hvp_backward_chi(chi, dchi) - whole).max() / np.abs(whole).max())

            def split(nv):
                _, ds = h.hvp_forward(V[:nv])
                h.hvp_backward(f_total, ds)

            def callers(nv):
                h.hvp_forward(V[:nv], final_states=True)
                h.hvp_backward_chi(chi, dchi[:nv])

            for nv in nvs:
                run[f"split_{nv}"] = (lambda nv=nv: split(nv))
                run[f"chi_{nv}"] = (lambda nv=nv: callers(nv))
        for fn in run.values():      # warm-up: module loads, the captured graph, the HVP storage
            fn()
            fn()
        res = {name: [] for name in run}
        for _ in range(a.rounds):
            for name, fn in run.items():
                per_direction = not name.endswith("_eval")
                if per_direction:
                    h.eval(x)
                res[name].append(timed(fn, a.reps) / (int(name.split("_")[1]) if per_direction else 1))
        bitwise = hvp_bitwise = None
        if a.old:
            (J0, G0, _), (J1, G1, _) = hs["old_eval"].eval(x), h.eval(x)
            bitwise = bool(J0 == J1 and np.array_equal(G0, G1))
            if hasattr(hs["old_eval"]._lib.grape_hvp, "__call__"):
                hvp_bitwise = bool(np.array_equal(hs["old_eval"].hvp(V), h.hvp(V)))
        h.eval(x)
        t0 = time.perf_counter()
        h.hvp(V[:max(nvs)])
        dt = time.perf_counter() - t0
        info = h.hvp_info()
        cus = min(256, pr["K"] * min(max(nvs), info["dirs_per_group"]))
        row = dict(shape=cid, N=N, L=L, N_T=pr["N_T"], K=pr["K"], rounds_ms=res, eval_bitwise=bitwise, hvp_bitwise=hvp_bitwise,
                   split_bitwise=split_bitwise, chi_rel=chi_rel, info=info,
                   terms_per_substep=info["series_terms"] / max(info["series_steps"], 1),
                   mfma_frac=mfma_flop(info, N, L) / dt / (cus * PEAK_PER_CU))
        print(json.dumps(row), flush=True)
        rows.append(row)
        for hh in hs.values():
            hh.close()
    names = list(rows[0]["rounds_ms"])
    print("# medians over the rounds in ms (spread = max - min of the rounds); hvp_<nv>: per direction")
    print("# shape N L N_T K | " + " | ".join(names) + " | eval bitwise | hvp bitwise | split bitwise | chi rel | terms / (sub-)step | mfma_frac")
    for r in rows:
        med = {n: float(np.median(r["rounds_ms"][n])) for n in names}
        spr = {n: max(r["rounds_ms"][n]) - min(r["rounds_ms"][n]) for n in names}
        print(f"{r['shape']} {r['N']} {r['L']} {r['N_T']} {r['K']} | " + " | ".join(f"{med[n]:.3f} ({spr[n]:.3f})" for n in names) +
              f" | {r['eval_bitwise']} | {r['hvp_bitwise']} | {r['split_bitwise']} | {r['chi_rel']} | {r['terms_per_substep']:.1f} | {r['mfma_frac']:.4f}")


if __name__ == "__main__":
    main()
