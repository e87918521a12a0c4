"""What grape_expect costs next to the route it replaces, and that grape_eval did not move against the parent commit -- ONE
process on one GPU.

  python tools/expect_ab.py [--old tools/_prev.so] [--M 1,4,16] [--rounds 3] [--reps 3] [--closed C3] [--open 32,8,1000]

Shapes: the closed configuration C3 of synth.CONFIGS (N = 64, K = 128, 1000 steps) and one open-system problem
synth.make_open_problem(d = 32, L = 2, 1000 steps, K = 8, J = 2).  Operators: tests' recipe (GUE plus the identity, unit 2-norm;
position 1 -- position 0 when alone -- non-Hermitian).  For every shape and every round, in this order:
  eval_old   grape_eval with a gradient on the library of the PARENT commit (--old; left out without it)
  eval_new   the same on the current library, before any grape_expect and again after all of them; J and G are compared bit
             for bit with the parent's, both times
  expect_M   one grape_expect call with M observables (host wall time of the call: upload of the operators, kernel, copy of
             the K (N_T+1) M results)
  host_M     the route it replaces: storage(0) -- the copy of all stored states -- plus numpy.einsum(..., optimize=True)
Each figure is ms, the minimum over --reps inside a round (host_M: one repetition); the table prints the median over the rounds
and the spread (max - min).  `values` is the largest deviation of the device's values from the host route's; `Gflop/s` is the
flop of the matrix instructions (grape_get_expect_info[3]) over the time of the WHOLE call, not a kernel rate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ab_lib  # noqa: E402
from open_ab import open_handle_of, timed  # noqa: E402
from grape_jl_amd import api, synth  # noqa: E402


def observables(N, M, seed):
    out = np.empty((M, N, N), complex)
    for m in range(M):
        s = synth.subseed(seed, 7000 + m)
        if m == (0 if M == 1 else 1):
            z = synth.normal(s, 2 * N * N)
            G = (z[0::2] + 1j * z[1::2]).reshape(N, N)
            O = G / np.linalg.norm(G, 2) + (0.8 + 0.6j) * np.eye(N)
        else:
            G = synth.gue(s, N)
            O = G / np.linalg.norm(G, 2) + (1.0 if m % 2 == 0 else -1.0) * np.eye(N)
        out[m] = O / np.linalg.norm(O, 2)
    return out


def host_route(h, ops, is_open):
    st = h.storage(0)
    if is_open:
        return np.einsum("mij,knji->knm", ops, st, optimize=True)
    return np.einsum("kni,mij,knj->knm", st.conj(), ops, st, optimize=True)


def same_bits(a, b):
    return bool(a[0] == b[0] and np.array_equal(a[1], b[1]))


def run_shape(label, pr, make, old_path, Ms, rounds, reps, is_open):
    x = pr["pulsevals"]
    N = pr["H0"].shape[-1]
    h_old = make(old_path, pr) if old_path else None
    h = make(api_new, pr)
    ev = lambda hh: hh.eval(x)[:2]   # noqa: E731
    ev(h)
    before = ev(h)                                             # (warm; the handle has not seen grape_expect yet)
    old = None
    if h_old:
        ev(h_old)
        old = ev(h_old)
    opss = {M: observables(N, M, 9000 + N) for M in Ms}
    res = {"eval_old": [], "eval_new": []}
    dev, flop = {}, {}
    for M in Ms:
        got = h.expect(opss[M])                                # (warm: allocation, code object)
        dev[M] = float(np.abs(got - host_route(h, opss[M], is_open)).max())
        flop[M] = h.expect_info()["mfma_flop"]
        res[f"expect_{M}"], res[f"host_{M}"] = [], []
    for _ in range(rounds):
        if h_old:
            res["eval_old"].append(timed(lambda: ev(h_old), reps))
        res["eval_new"].append(timed(lambda: ev(h), reps))
        for M in Ms:
            res[f"expect_{M}"].append(timed(lambda: h.expect(opss[M]), reps))
            res[f"host_{M}"].append(timed(lambda: host_route(h, opss[M], is_open), 1))
    after = ev(h)
    row = dict(shape=label, N=N, K=pr["H0"].shape[0], steps=len(pr["tlist"]) - 1, rounds_ms={k: v for k, v in res.items() if v},
               values_max_dev=dev, mfma_flop=flop, bytes=h.expect_info()["bytes"],
               eval_same_bits_after_expect=same_bits(after, before))
    if old:
        row["eval_same_bits_as_old"] = same_bits(before, old) and same_bits(after, old)
    print(json.dumps(row), flush=True)
    for hh in (h, h_old):
        if hh:
            hh.close()
    return row


def main():
    global api_new
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="library built from the parent commit")
    ap.add_argument("--M", default="1,4,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--closed", default="C3")
    ap.add_argument("--open", default="32,8,1000", help="d,K,steps")
    a = ap.parse_args()
    api_new = api.library_path()
    Ms = [int(m) for m in a.M.split(",") if m]
    rows = [run_shape(a.closed, synth.make_config(a.closed), ab_lib.handle_of, a.old, Ms, a.rounds, a.reps, False)]
    d, K, steps = [int(v) for v in a.open.split(",")]
    pr = synth.make_open_problem(d, 2, steps, K, 2, seed=synth.BASE_SEED ^ (1000 + d))
    rows.append(run_shape(f"open d={d} K={K}", pr, open_handle_of, a.old, Ms, a.rounds, a.reps, True))
    print("# medians over the rounds in ms (spread = max - min of the rounds); host = storage(0) + numpy.einsum")
    print("# shape | eval_old | eval_new | J, G same bits as old (before and after expect) | M | expect | host | host / expect | values | Gflop/s of the call")
    for r in rows:
        med = {n: float(np.median(v)) for n, v in r["rounds_ms"].items()}
        spr = {n: max(v) - min(v) for n, v in r["rounds_ms"].items()}
        cell = lambda n: f"{med[n]:.2f} ({spr[n]:.2f})" if n in med else "-"   # noqa: E731
        for M in Ms:
            e, hst = f"expect_{M}", f"host_{M}"
            print(f"{r['shape']} N={r['N']} K={r['K']} steps={r['steps']} | {cell('eval_old')} | {cell('eval_new')} | "
                  f"{r.get('eval_same_bits_as_old', '-')} | {M} | {cell(e)} | {cell(hst)} | {med[hst] / med[e]:.1f} | "
                  f"{r['values_max_dev'][M]:.1e} | {r['mfma_flop'][M] / med[e] * 1e-6:.0f}")


if __name__ == "__main__":
    main()
