"""Open-system GRAPE: the native route (GrapeHipOpen: d x d density matrices in matrix form) against the vectorised route
(GrapeHip on the d^2 x d^2 Liouvillian) of the same build, same problem, in ONE process on one GPU.

  python tools/open_ab.py [--old tools/_prev.so] [--d 4,8,12,16] [--native-only 32,48,64] [--K 1,8] [--steps 500]
                          [--rounds 3] [--reps 3]

Problem: synth.make_open_problem(d, L = 2, steps, K, J = 2), dt = 1 (||H|| dt ~ 1).  For every (d, K) and every round, in this
order (old first, as the other A/B records of the project):
  vec_old   grape_eval on liouvillian(...) with the library of the PARENT commit (--old; left out without it)
  vec       the same on the current library -- must not move against vec_old by more than their run-to-run spread
  native    GrapeHipOpen of the current library
Each figure is ms per evaluation with a gradient (host wall time, minimum over --reps inside the round); the table prints
the median over the rounds and the spread (max - min).  Also printed: device bytes the handle holds (free device memory
before creation minus after the first evaluation), series terms per (sub-)step and sub-steps per step of the native route,
and the flop of the matrix instructions it EXECUTED per second of its launch as a fraction of the peak of the CUs that launch
occupies (78.6 TF/s / 256 per CU; K workgroups forward, K L backward)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ab_lib  # noqa: E402
from ab_lib import handle_of  # noqa: E402
import grape_jl_amd as g  # noqa: E402
from grape_jl_amd import api, synth  # noqa: E402

PEAK_PER_CU = 78.6e12 / 256


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def open_handle_of(path, pr):
    api._lib = None
    api.library_path = (lambda p: (lambda: p))(os.path.abspath(path))
    saved, ctypes.CDLL = ctypes.CDLL, ab_lib._TolerantCDLL
    try:
        return g.GrapeHipOpen(pr["H0"], pr["Hc"], pr["cops"], pr["tlist"], pr["rho0"], pr["target"], pr["weights"])
    finally:
        ctypes.CDLL = saved


def vectorised(pr):
    K, L = pr["H0"].shape[0], pr["Hc"].shape[0]
    vec = lambda r: np.swapaxes(r, -1, -2).reshape(r.shape[0], -1)   # noqa: E731
    return dict(H0=np.stack([g.liouvillian(pr["H0"][k], pr["cops"]) for k in range(K)]),
                Hc=np.stack([g.liouvillian(pr["Hc"][l]) for l in range(L)]), tlist=pr["tlist"], psi0=vec(pr["rho0"]),
                target=vec(pr["target"]), weights=pr["weights"])


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit (baseline of the vectorised rows)")
    ap.add_argument("--d", default="4,8,12,16")
    ap.add_argument("--native-only", default="32,48,64")
    ap.add_argument("--K", default="1,8")
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    new = api.library_path()
    both = [int(x) for x in a.d.split(",") if x]
    alone = [int(x) for x in a.native_only.split(",") if x]
    rows = []
    for d in both + alone:
        for K in [int(x) for x in a.K.split(",")]:
            pr = synth.make_open_problem(d, 2, a.steps, K, 2, seed=synth.BASE_SEED ^ (1000 + d))
            x = pr["pulsevals"]
            hs, held = {}, {}
            if d in both:
                pv = vectorised(pr)
                if a.old:
                    hs["vec_old"] = handle_of(a.old, pv)
                f0 = free_bytes()
                hs["vec"] = handle_of(new, pv)
                hs["vec"].eval(x)
                held["vec"] = f0 - free_bytes()
            f0 = free_bytes()
            hs["native"] = open_handle_of(new, pr)
            hs["native"].eval(x)
            held["native"] = f0 - free_bytes()
            reps = a.reps if d <= 16 else max(1, a.reps - 1)
            for h in hs.values():
                h.eval(x)
            res = {name: [] for name in hs}
            for _ in range(a.rounds if d <= 16 else max(1, a.rounds - 1)):
                for name, h in hs.items():
                    res[name].append(timed(lambda h=h: h.eval(x), reps))
            hn = hs["native"]
            hn.reset_timings()
            Jn, Gn, _ = hn.eval(x)
            t, w = hn.timings(), hn.work()
            L = 2
            fwd_steps = K * a.steps
            row = dict(d=d, N=d * d, K=K, steps=a.steps, rounds_ms=res, bytes=held,
                       terms_per_substep=w["series_terms"] / w["series_steps"], substeps_per_step=w["series_steps"] / (2.0 * fwd_steps),
                       native_forward_ms=t["forward"], native_backward_ms=t["backward"],
                       mfma_frac_forward=w["mfma_flop_forward"] / (t["forward"] * 1e-3) / (K * PEAK_PER_CU),
                       mfma_frac_backward=w["mfma_flop_backward"] / (t["backward"] * 1e-3) / (K * L * PEAK_PER_CU))
            if "vec" in hs:
                Jv, Gv, _ = hs["vec"].eval(x)
                row["dJ"], row["dG"] = abs(Jn - Jv), float(np.abs(Gn - Gv).max())
                row["vec_work"] = {k: v for k, v in hs["vec"].work().items() if k in ("matrix_free_fallback", "series_terms")}
            print(json.dumps(row), flush=True)
            rows.append(row)
            for h in hs.values():
                h.close()
    print("# medians over the rounds, ms per evaluation (spread = max - min of the rounds); bytes held on the device; native route:")
    print("# terms per (sub-)step, sub-steps per step, executed MFMA flop / time as a fraction of the peak of the occupied CUs (fwd, bwd)")
    print("# d N K | vec_old | vec | native | vec / native | MB vec | MB native | terms | substeps | frac fwd | frac bwd")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        cell = lambda n: f"{med[n]:.2f} ({spr[n]:.2f})" if n in med else "-"   # noqa: E731
        ratio = f"{med['vec'] / med['native']:.2f}" if "vec" in med else "-"
        mb = lambda n: f"{r['bytes'][n] / 1048576.0:.0f}" if n in r["bytes"] else "-"   # noqa: E731
        print(f"{r['d']} {r['N']} {r['K']} | {cell('vec_old')} | {cell('vec')} | {cell('native')} | {ratio} | {mb('vec')} | {mb('native')} | "
              f"{r['terms_per_substep']:.1f} | {r['substeps_per_step']:.2f} | {r['mfma_frac_forward']:.3f} | {r['mfma_frac_backward']:.3f}")


if __name__ == "__main__":
    main()
