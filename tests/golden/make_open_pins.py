#!/usr/bin/env python3
"""Regenerates tests/golden/open_pin_{d33,d48,d64}.json: the open-system evaluation (grape_create_open) at the sizes of the
NP = 48 and NP = 64 kernels, by the plain matrix-form reference of tests/open_reference.py run in x87 long double
(numpy.clongdouble, eps = 1.1e-19; series summed until a term is below 1e-24 of the sum), printed to 25 digits:
J, tau, G and tau_grads of the three built-in functionals.  rho(T) is left out: it alone would be larger than any fixture
of this folder.  The inputs are regenerated from the synth seeds in the file (tests/open_helpers.py: open_pin_problem).

The CPU suite checks that the double-precision reference reproduces each pin to 1e-14 (tests/test_open_reference.py), the
GPU suite compares the kernels with the pins (tests/test_gpu_open_reference.py).

Run from the repository root; numpy has no BLAS for long double (a 64 x 64 product takes 3.5 ms), so d33 takes about
8 s, d48 about 15 s and d64 about 90 s:
    python tests/golden/make_open_pins.py [d33 d48 d64]
"""
import json
import os
import sys
import time

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.dirname(OUT)]
import open_helpers as oh  # noqa: E402
import open_reference as orf  # noqa: E402


def s(x):
    return np.format_float_scientific(np.longdouble(x), precision=24, unique=False)


def main():
    assert np.finfo(np.longdouble).eps < 2e-19, "this platform's long double is not the x87 extended format"
    for name, spec in oh.PIN_SPECS.items():
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        t0 = time.time()
        pr = oh.open_pin_problem(spec)
        parts = orf.propagate(pr, pr["pulsevals"], dtype=np.clongdouble)
        out = dict(note="inputs: open_helpers.open_pin_problem(spec); outputs: tests/open_reference.py in numpy.clongdouble "
                        "(tests/golden/make_open_pins.py), printed to 25 digits", name=name, spec=spec, L=2, N_T=3, functionals={})
        for functional in (0, 1, 2):
            r = orf.from_parts(parts, pr, functional)
            c2 = lambda a: [s(a.real), s(a.imag)]   # noqa: E731
            out["functionals"][str(functional)] = dict(
                J=s(r["J"]), tau=[c2(t) for t in r["tau"]], G=[s(x) for x in r["G"]],
                tau_grads=[[[c2(z) for z in row] for row in per_k] for per_k in r["tau_grads"]])
        with open(os.path.join(OUT, f"open_pin_{name}.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(f"{name}: {time.time() - t0:.1f} s, J_sm = {out['functionals']['0']['J']}", flush=True)


if __name__ == "__main__":
    main()
