"""Time gradient and time-grid updates (ABI v7), the parts that run without a GPU: the exported symbols, the ABI version
that grape_create accepts, the all-reduce of ShardedEvaluator.time_gradient over two gloo ranks, and the oracle identity
that the GPU tests (tests/test_gpu_time_grid.py) compare against:

    dt_n dJ/d(dt_n) = G^c_n + sum_l eps_nl G_nl

where G^c is the gradient for a pseudo-control with operator H0_k and pulse value 1 (drift H0' = 0): scaling dt_n by
(1 + s) scales every term of H_n dt_n, i.e. every control value of interval n including the pseudo-control's."""
import ctypes
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from grape_jl_amd import synth
from grape_jl_amd.sharded import ShardedEvaluator, shard_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pseudo_control_dJdt(ref, H0, Hc, tlist, pulsevals, psi0, target, weights=None, functional=0,
                        gradient_method=0, D=None, lambda_b=1.0):
    """dJ/d(dt_n) from the oracle's gradient with the drift as a pseudo-control (the propagation part only: with a running
    cost the explicit derivative of the trapezoid weights is not in it)."""
    H0 = np.asarray(H0)
    Hc = np.asarray(Hc)
    K, N = H0.shape[0], H0.shape[1]
    Hck = Hc if Hc.ndim == 4 else np.broadcast_to(Hc, (K,) + Hc.shape)
    L = Hck.shape[1]
    Hp = np.concatenate([H0[:, None], Hck], axis=1)
    N_T = len(tlist) - 1
    x = np.concatenate([np.ones(N_T), np.asarray(pulsevals, dtype=np.float64)])
    kw = dict(weights=weights, functional=functional, gradient_method=gradient_method)
    if D is not None:
        kw.update(D=D, lambda_b=lambda_b)
    _, G, _ = ref.evaluate(np.zeros((K, N, N), complex), Hp, tlist, x, psi0, target, **kw)
    G = G.reshape(L + 1, N_T)
    eps = np.asarray(pulsevals).reshape(L, N_T)
    return (G[0] + np.sum(eps * G[1:], axis=0)) / np.diff(tlist)


def running_cost_weight_term(ref, H0, Hc, tlist, pulsevals, psi0, D, lambda_b):
    """lambda_b / 2 sum_k (g_b,k(t_n) + g_b,k(t_{n+1})) of interval n, g_b = <Psi|D|Psi> (optimize.jl:727-750)."""
    H0, Hc = np.asarray(H0), np.asarray(Hc)
    K, N = H0.shape[0], H0.shape[1]
    L = Hc.shape[-3]
    N_T = len(tlist) - 1
    eps = np.asarray(pulsevals).reshape(L, N_T)
    dts = np.diff(tlist)
    g = np.zeros((K, N_T + 1))
    for k in range(K):
        Hk = Hc[k] if Hc.ndim == 4 else Hc
        Dk = D[k] if np.ndim(D) == 3 else D
        psi = np.asarray(psi0[k], dtype=complex)
        g[k, 0] = np.real(np.vdot(psi, Dk @ psi))
        for n in range(N_T):
            H = H0[k] + np.tensordot(eps[:, n], Hk, axes=1)
            psi = ref.expm(-1j * dts[n] * H)[0] @ psi
            g[k, n + 1] = np.real(np.vdot(psi, Dk @ psi))
    return 0.5 * lambda_b * np.sum(g[:, :-1] + g[:, 1:], axis=0)


def central_dJdt(ref, H0, Hc, tlist, pulsevals, psi0, target, weights=None, functional=0, D=None, lambda_b=1.0, rel=1e-5):
    """Central differences of the oracle's J in dt_n: shifting dt_n shifts every later grid point."""
    N_T = len(tlist) - 1
    out = np.empty(N_T)
    kw = dict(weights=weights, functional=functional, gradient=False)
    if D is not None:
        kw.update(D=D, lambda_b=lambda_b)
    for n in range(N_T):
        h = rel * (tlist[n + 1] - tlist[n])
        tp, tm = np.array(tlist, dtype=float), np.array(tlist, dtype=float)
        tp[n + 1:] += h
        tm[n + 1:] -= h
        Jp = ref.evaluate(H0, Hc, tp, pulsevals, psi0, target, **kw)[0]
        Jm = ref.evaluate(H0, Hc, tm, pulsevals, psi0, target, **kw)[0]
        out[n] = (Jp - Jm) / (2 * h)
    return out


def _nonuniform(pr, seed=5):
    N_T = len(pr["tlist"]) - 1
    u = synth.uniform01(seed, N_T)
    return np.concatenate([[0.0], np.cumsum(0.3 + 0.4 * u)])


def test_library_exports_the_v7_entry_points():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    lib = ctypes.CDLL(api.library_path())
    for name in ("grape_get_time_gradient", "grape_set_tlist"):
        assert hasattr(lib, name) and name in api.EXPORTS
    lib.grape_abi_version.restype = ctypes.c_int
    assert api.ABI_VERSION == 7 and lib.grape_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert "#define GRAPE_HIP_ABI_VERSION 7" in hdr
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    assert "const ABI_VERSION = 7" in jl and "grape_get_time_gradient" in jl and "grape_set_tlist" in jl


def test_v6_problems_still_reach_validation():
    """grape_problem did not change in v7: a struct with abi_version 6 passes the version check and meets the argument
    validation behind it (before any HIP call); 99 does not."""
    from grape_jl_amd import api
    lib = api.load_library()
    h = ctypes.c_void_p()
    p = api._Problem()
    p.abi_version, p.N, p.K, p.N_T, p.L = 6, 4, 1, 3, 0
    assert lib.grape_create(ctypes.byref(h), ctypes.byref(p)) == -6   # "no controls": past the version check
    assert b"no controls" in lib.grape_last_error(None)
    p.abi_version = 99
    assert lib.grape_create(ctypes.byref(h), ctypes.byref(p)) == -1
    assert b"abi_version" in lib.grape_last_error(None)
    p.abi_version, p.L = 6, 1
    tl = np.array([0.0, 1.0, 1.0, 2.0])   # not strictly increasing: refused by the validation of v6 and v7 alike
    z = np.zeros((1, 4, 4), complex)
    psi = np.ones((1, 4), complex)
    p.tlist, p.H0, p.Hc, p.psi0, p.target = tl.ctypes.data, z.ctypes.data, z.ctypes.data, psi.ctypes.data, psi.ctypes.data
    assert lib.grape_create(ctypes.byref(h), ctypes.byref(p)) == -1
    assert b"strictly increasing" in lib.grape_last_error(None)


def test_new_entry_points_refuse_null_handles():
    from grape_jl_amd import api
    lib = api.load_library()
    buf = np.zeros(4)
    assert lib.grape_get_time_gradient(None, buf.ctypes.data) == -1
    assert lib.grape_set_tlist(None, buf.ctypes.data) == -1


def test_new_kernel_has_no_scratch(tmp_path):
    """The time-gradient kernel keeps everything in registers and the LDS: no scratch (private memory) on gfx950."""
    src = tmp_path / "tg.hip"
    src.write_text('#include "grape_kernels.hip.h"\n#include "grape_timegrad.hip.h"\n'
                   "template __global__ void time_grad_kernel<1>(TimeGradArgs);\n"
                   "template __global__ void time_grad_kernel<2>(TimeGradArgs);\n"
                   "template __global__ void time_grad_kernel<4>(TimeGradArgs);\n")
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "tg.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    blocks = res.stderr.split("Function Name: ")
    seen = 0
    for b in blocks[1:]:
        if "time_grad_kernel" not in b.splitlines()[0]:
            continue
        seen += 1
        scratch = [re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln) for ln in b.splitlines()]
        scratch = [int(m.group(1)) for m in scratch if m]
        assert scratch == [0], b[:1500]
    assert seen == 3, res.stderr[-2000:]


@pytest.mark.parametrize("functional", [0, 1, 2])
def test_pseudo_control_identity_against_central_differences(ref, functional):
    pr = synth.make_problem(6, 2, 7, 3, seed=21)
    tl = _nonuniform(pr)
    w = np.array([0.5, 1.0, 1.5])
    args = (pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], pr["target"])
    got = pseudo_control_dJdt(ref, *args, weights=w, functional=functional)
    fd = central_dJdt(ref, *args, weights=w, functional=functional)
    assert np.abs(got - fd).max() <= 1e-8 * max(np.abs(fd).max(), 1e-3), (got, fd)


def test_pseudo_control_identity_per_trajectory_controls(ref):
    pr = synth.make_problem(5, 1, 6, 2, seed=8)
    Hc = np.stack([pr["Hc"], 1.3 * pr["Hc"]])   # [K, L, N, N]
    tl = _nonuniform(pr, seed=9)
    args = (pr["H0"], Hc, tl, pr["pulsevals"], pr["psi0"], pr["target"])
    got = pseudo_control_dJdt(ref, *args, functional=1)
    fd = central_dJdt(ref, *args, functional=1)
    assert np.abs(got - fd).max() <= 1e-8 * max(np.abs(fd).max(), 1e-3)


def test_pseudo_control_identity_with_running_cost(ref):
    """With D / lambda_b the identity gives dJ/d(dt_n) minus the explicit derivative of the trapezoid weights."""
    pr = synth.make_problem(5, 2, 6, 2, seed=13)
    N = 5
    X = synth.normal(77, 2 * N * N).reshape(2, N, N)
    Dm = (X[0] + 1j * X[1]) / 4
    Dm = Dm + Dm.conj().T
    tl = _nonuniform(pr, seed=3)
    args = (pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], pr["target"])
    lam = 0.3
    prop = pseudo_control_dJdt(ref, *args, D=Dm, lambda_b=lam)
    expl = running_cost_weight_term(ref, pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], Dm, lam)
    fd = central_dJdt(ref, *args, D=Dm, lambda_b=lam)
    assert np.abs(expl).max() > 1e-3   # (the term is not negligible here)
    assert np.abs(prop + expl - fd).max() <= 1e-8 * max(np.abs(fd).max(), 1e-3)


def intervals_per_workgroup(NP):
    """CW = 16 nct of time_grad_kernel: `const int nct = h->NP <= 64 ? 4 : h->NP <= 128 ? 2 : 1;` in grape_get_time_gradient
    (csrc/grape_hip.hip), restated.  LONG_CASES is chosen by it: the two move together."""
    return 16 * (4 if NP <= 64 else 2 if NP <= 128 else 1)


def padded_size(N):
    """NP of a handle with the default propagator (grape_create, csrc/grape_hip.hip): 16-wide tiles up to 64, then 128 / 256 / 512"""
    return 16 * ((N + 15) // 16) if N <= 64 else 128 if N <= 128 else 256 if N <= 256 else 512


# Time grids beyond the first workgroup of time_grad_kernel (the GPU side is tests/test_gpu_time_grid.py): n0 > 0, the guarded
# tail of the last block, the g_b read and the reduction across block boundaries.
LONG_CASES = [
    # id, N, L, K, N_T, functional, hermitian, blocks = ceil(N_T / CW)
    ("n16-one-full-block", 16, 2, 3, 64, 0, True, 1),      # CW = 64, exactly full: the boundary without a tail
    ("n16-one-column-over", 16, 2, 3, 65, 1, True, 2),     # the last block holds one interval, 63 guarded columns
    ("n33-three-blocks", 33, 2, 2, 130, 2, False, 3),      # NP = 48: padded rows, three of the four waves have a row tile
    ("n64-one-column-over", 64, 2, 2, 65, 0, True, 2),     # the headline route (asm_kernel == 1)
    ("n64-three-blocks", 64, 2, 2, 130, 1, True, 3),
    ("n100-two-blocks", 100, 1, 2, 33, 0, True, 2),        # nct = 2, CW = 32, a tail of 1
    ("n65-three-blocks", 65, 1, 2, 70, 2, False, 3),       # the smallest N padded to 128, a tail of 6
    ("n130-two-blocks", 130, 1, 1, 17, 0, True, 2),        # nct = 1, CW = 16, a tail of 1
    ("n129-three-blocks", 129, 1, 1, 35, 1, True, 3),      # a tail of 3
]
LONG_IDS = [c[0] for c in LONG_CASES]
_long = {}


def long_grid(N_T, seed):
    """the non-uniform grid of the GPU tests (``_nonuniform`` of tests/test_gpu_time_grid.py)"""
    u = synth.uniform01(seed, N_T)
    return np.concatenate([[0.0], np.cumsum(0.3 + 0.4 * u)])


def long_case(ref, cid):
    """(problem, grid, weights, the oracle's dJ/d(dt_n)) of a LONG_CASES entry, built as test_against_the_oracle builds its
    cases.  Computed once per session and shared; nobody writes to it."""
    if cid not in _long:
        _, N, L, K, N_T, fn, herm, _ = LONG_CASES[LONG_IDS.index(cid)]
        pr = synth.make_problem(N, L, N_T, K, seed=31 + N, hermitian=herm)
        tl = long_grid(N_T, seed=N)
        w = np.linspace(0.5, 1.5, K)
        want = pseudo_control_dJdt(ref, pr["H0"], pr["Hc"], tl, pr["pulsevals"], pr["psi0"], pr["target"], weights=w,
                                   functional=fn)
        want.setflags(write=False)
        _long[cid] = (pr, tl, w, want)
    return _long[cid]


def assert_every_block_has_signal(want, CW, label=""):
    """On the reference alone: every block of CW intervals reaches 1e-3, the floor of the bar.  An error confined to a later
    block can then hide neither under the first block's scale nor under the floor."""
    peaks = [float(np.abs(want[b:b + CW]).max()) for b in range(0, len(want), CW)]
    print(label, dict(block_peaks=peaks, overall=float(np.abs(want).max())))
    assert min(peaks) >= 1e-3, (label, peaks)
    return peaks


@pytest.mark.parametrize("cid", LONG_IDS)
def test_long_cases_cross_blocks_and_every_block_has_signal(ref, cid):
    _, N, L, K, N_T, fn, herm, blocks = LONG_CASES[LONG_IDS.index(cid)]
    CW = intervals_per_workgroup(padded_size(N))
    assert -(-N_T // CW) == blocks, (N_T, CW)
    _, _, _, want = long_case(ref, cid)
    assert want.shape == (N_T,) and np.all(np.isfinite(want))
    assert len(assert_every_block_has_signal(want, CW, cid)) == blocks


def test_the_block_rule_is_the_launch_code():
    """intervals_per_workgroup and padded_size against the lines of csrc/grape_hip.hip they restate"""
    src = open(os.path.join(ROOT, "grape.jl_amd", "csrc", "grape_hip.hip")).read()
    assert "const int nct = h->NP <= 64 ? 4 : h->NP <= 128 ? 2 : 1;" in src
    assert "const dim3 grid((unsigned)((N_T + 16 * nct - 1) / (16 * nct)), (unsigned)h->K);" in src
    assert "h->NP = p->N <= 128 ? 128 : (p->N <= 256 ? 256 : 512)" in src
    assert [intervals_per_workgroup(p) for p in (16, 48, 64, 128, 256, 512)] == [64, 64, 64, 32, 16, 16]
    assert [padded_size(n) for n in (16, 17, 33, 64, 65, 128, 129, 256, 257)] == [16, 32, 48, 64, 128, 128, 256, 256, 512]


class _FakeShard:
    """Split-phase stand-in with a fixed partial time gradient and a record of the grids it was given."""

    def __init__(self, part):
        self.part, self.grids = part, []

    def time_gradient(self):
        return self.part

    def set_tlist(self, tlist):
        self.grids.append(np.array(tlist))


def _tg_worker(rank, world, port, q):
    # every way out reports to the parent (an exception in one rank must not leave the parent waiting for ever), and the
    # collectives give up after a minute instead of gloo's default half hour
    import datetime
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        part = np.arange(5, dtype=float) * (rank + 1) + 0.25 * rank
        fake = _FakeShard(part)
        ev = ShardedEvaluator(fake, 4, 0, dist=dist)
        ev.set_tlist(np.linspace(0, 2, 6))
        q.put((rank, ev.time_gradient().tolist(), len(fake.grids)))
        dist.barrier()
        dist.destroy_process_group()
    except BaseException as e:   # noqa: BLE001 -- reported to the parent, which fails the test
        q.put((rank, "error", repr(e)))


def test_two_rank_gloo_time_gradient_is_all_reduced():
    import queue
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tg_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = []
    try:
        for _ in range(2):
            got.append(q.get(timeout=180))
    except queue.Empty:
        pass
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.kill()
                p.join(10)
    got.sort(key=lambda r: r[0])
    want = (np.arange(5) * 1.0 + np.arange(5) * 2.0 + 0.25).tolist()
    assert got == [(0, want, 1), (1, want, 1)], got
    assert all(p.exitcode == 0 for p in procs)
    assert shard_range(4, 2, 0) == (0, 2)
    _ = torch
