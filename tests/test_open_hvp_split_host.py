"""grape_open_hvp_forward / grape_open_hvp_backward / grape_open_hvp_backward_chi (csrc/grape_lindblad_hvp_split.hip.h,
DESIGN.md 22) -- what can be checked without a GPU: the entry points through every layer (header, export list, ctypes binding,
Julia glue), the refusals that come before the first HIP call, the shape checks of the Python methods, the resource usage of
the four instantiations of the new sweep kernel, and the protocol of ShardedEvaluator.hvp_host on stub open shards."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hvp_split_host import StubShard, SumOfShards  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = (r"int grape_open_hvp_forward\(grape_handle \*h, int nv, const double \*V, double \*dtau, double \*dsums, double \*drhoT\);",
         r"int grape_open_hvp_backward\(grape_handle \*h, int nv, const double f_total\[2\], const double \*df_total, double \*HV\);",
         r"int grape_open_hvp_backward_chi\(grape_handle \*h, int nv, const double \*chi, const double \*dchi, double \*HV\);")
NAMES = ("grape_open_hvp_forward", "grape_open_hvp_backward", "grape_open_hvp_backward_chi")


def test_entry_points_are_declared_exported_bound_and_called_from_julia():
    from grape_jl_amd import api
    header = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    for d in DECLS:
        assert re.search("^" + d, header, re.M), d
    assert "#define GRAPE_HIP_ABI_VERSION 7" in header                  # entry points only
    for n in NAMES:
        assert n in api.EXPORTS
    for m in ("open_hvp_forward", "open_hvp_backward", "open_hvp_backward_chi"):
        assert callable(getattr(api.GrapeHipOpen, m))
        assert not hasattr(api.GrapeHip, m)                             # (ShardedEvaluator.hvp_host chooses by these names)
    julia = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for fn in ("function open_hvp_forward!(h::Handle, V::VecOrMat{Float64};", "function open_hvp_backward!(HV::VecOrMat{Float64}, h::Handle,",
               "function open_hvp_backward_chi!(HV::VecOrMat{Float64}, h::Handle,"):
        assert fn in julia, fn
    for n in NAMES:
        assert "ccall((:%s, libgrape), Cint" % n in julia, n


def test_null_arguments_and_closed_handles_are_refused_with_a_message():
    import __graft_entry__ as entry
    from test_hvp_split_host import _tiny_problem
    entry.build()
    from grape_jl_amd import api
    lib = api.load_library()
    vp, ip = ctypes.c_void_p, ctypes.c_int
    assert lib.grape_open_hvp_forward.argtypes == [vp, ip, vp, vp, vp, vp]
    assert lib.grape_open_hvp_backward.argtypes == [vp, ip, vp, vp, vp]
    assert lib.grape_open_hvp_backward_chi.argtypes == [vp, ip, vp, vp, vp]
    a = np.zeros(64)
    d = a.ctypes.data
    assert lib.grape_open_hvp_forward(None, 1, d, None, None, None) == -1
    assert b"grape_open_hvp_forward: h == NULL" in lib.grape_last_error(None)
    assert lib.grape_open_hvp_backward(None, 1, d, d, d) == -1
    assert b"grape_open_hvp_backward: h == NULL" in lib.grape_last_error(None)
    assert lib.grape_open_hvp_backward_chi(None, 1, d, d, d) == -1
    assert b"grape_open_hvp_backward_chi: h == NULL" in lib.grape_last_error(None)
    # with a (closed) handle, where a device exists: the argument checks, then the refusal of a closed handle
    p, keep = _tiny_problem(api)
    h = ctypes.c_void_p()
    rc = lib.grape_create(ctypes.byref(h), ctypes.byref(p))
    assert rc in (0, -2), (rc, lib.grape_last_error(None))
    if rc == 0:
        for nv, v in ((0, d), (1, None)):
            assert lib.grape_open_hvp_forward(h, nv, v, None, None, None) == -1
            assert b"grape_open_hvp_forward: nv must be positive, V must not be NULL" in lib.grape_last_error(h)
        for args in ((0, d, d, d), (1, None, d, d), (1, d, None, d), (1, d, d, None)):
            assert lib.grape_open_hvp_backward(h, *args) == -1
            assert b"grape_open_hvp_backward: nv must be positive, f_total, df_total and HV must not be NULL" in lib.grape_last_error(h)
            assert lib.grape_open_hvp_backward_chi(h, *args) == -1
            assert b"grape_open_hvp_backward_chi: nv must be positive, chi, dchi and HV must not be NULL" in lib.grape_last_error(h)
        for call in (lambda: lib.grape_open_hvp_forward(h, 1, d, None, None, None), lambda: lib.grape_open_hvp_backward(h, 1, d, d, d),
                     lambda: lib.grape_open_hvp_backward_chi(h, 1, d, d, d)):
            assert call() == -1
            msg = lib.grape_last_error(h)
            assert b"not an open-system handle" in msg and b"grape_hvp_forward" in msg
        lib.grape_destroy(h)
    _ = keep


def _bare():
    """an instance without a handle: the shape checks come before any call into the library"""
    from grape_jl_amd import api
    h = api.GrapeHipOpen.__new__(api.GrapeHipOpen)
    h.L, h.N_T, h.K, h.N, h._h = 2, 3, 2, 4, None
    return h


def test_the_python_methods_check_their_shapes():
    h = _bare()
    for bad in (np.zeros(5), np.zeros((2, 5)), np.zeros((0, 6)), np.zeros((1, 2, 3)), np.zeros(())):
        with pytest.raises(ValueError, match=r"V must be \[L\*N_T\] = \[6\]"):
            h.open_hvp_forward(bad)
    for bad in (np.zeros((2, 2), complex), np.zeros(0, complex)):
        with pytest.raises(ValueError, match="df_total must be"):
            h.open_hvp_backward(1.0 + 0j, bad)
    chi = np.zeros((2, 4, 4), complex)
    for bad in (np.zeros((2, 4), complex), np.zeros((2, 4, 5), complex), np.zeros((1, 4, 4), complex)):
        with pytest.raises(ValueError, match=r"chi must be \[K, d, d\] = \[2, 4, 4\]"):
            h.open_hvp_backward_chi(bad, chi)
    for bad in (np.zeros((2, 4, 5), complex), np.zeros((3, 2, 4, 5), complex), np.zeros((0, 2, 4, 4), complex), np.zeros(32, complex),
                np.zeros((1, 1, 2, 4, 4), complex), np.zeros((2, 4), complex)):
        with pytest.raises(ValueError, match="dchi must be"):
            h.open_hvp_backward_chi(chi, bad)


def test_new_header_is_a_build_source_and_the_old_one_is_untouched():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_lindblad_hvp_split.hip.h") in srcs
    main = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_lindblad_hvp_split.hip.h"' in main
    old = open(os.path.join(api._CSRC, "grape_lindblad_hvp.hip.h")).read()
    assert "split" not in old and "chi_kernel" not in old          # the set of kernels there does not change


def test_backward_chi_kernels_have_no_scratch(tmp_path):
    """The four instantiations of lind_hvp_backward_chi_kernel keep what lind_hvp_backward_kernel keeps: no scratch (private
    memory) on gfx950 and no more LDS than the original at the same NP (red[2][8][NW] and nothing else).  Measured (printed
    here): VGPRs 89 / 97 / 111 / 156 at NP = 16 / 32 / 48 / 64 (the original: 90 / 98 / 110 / 156), LDS 128 / 512 /
    1152 / 1024 bytes for both."""
    src = tmp_path / "lind_hvp_split.hip"
    inst = "".join(f"template __global__ void lind_hvp_backward_chi_kernel<{np_}>(LindHvpArgs, const double *, const double *);\n"
                   f"template __global__ void lind_hvp_backward_kernel<{np_}>(LindHvpArgs);\n" for np_ in (16, 32, 48, 64))
    src.write_text('#include "grape_lindblad_hvp_split.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "lind_hvp_split.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for b in res.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_Z2\dlind_hvp_backward_(chi_)?kernelILi(\d+)EEv11LindHvpArgs", b)
        if not m:
            continue
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)]
        vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", b)]
        lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", b)]
        assert scratch == [0], b[:1500]
        seen[("chi" if m.group(1) else "builtin", int(m.group(2)))] = (vgprs[0], lds[0])
    print(dict(vgprs_lds=seen))
    assert sorted(seen) == [(kind, np_) for kind in ("builtin", "chi") for np_ in (16, 32, 48, 64)], res.stderr[-2000:]
    for np_ in (16, 32, 48, 64):
        assert seen[("chi", np_)][1] <= seen[("builtin", np_)][1]
        assert seen[("chi", np_)][0] <= 256                        # (two waves per SIMD at the least: 512 registers per lane)


class OpenStubShard(StubShard):
    """the stub of tests/test_hvp_split_host.py as an open shard: the product goes through open_hvp_forward / open_hvp_backward,
    and the closed methods -- which GrapeHipOpen inherits, and which refuse an open handle -- must not be called"""
    def open_hvp_forward(self, V):
        self.calls.append("open_hvp_forward")
        self.V = np.asarray(V, float)
        dtau = self.a[None, :] * self.V.sum(axis=-1, keepdims=True) * (1 + 2j)
        return dtau, (dtau * self._weights[None, :]).sum(axis=1)

    def hvp_forward(self, V):
        raise AssertionError("hvp_forward called on an open shard")

    def open_hvp_backward(self, f_total, df_total):
        self.calls.append("open_hvp_backward")
        self.got = (complex(f_total), np.array(df_total))
        return complex(f_total).imag * np.real(df_total)[:, None] * np.ones(self.LN) + self.a.sum() * self.V

    def hvp_backward(self, f_total, df_total):
        raise AssertionError("hvp_backward called on an open shard")


def test_sharded_hvp_host_on_stub_open_shards():
    from grape_jl_amd.sharded import ShardedEvaluator
    LN = 6
    V = np.arange(12.0).reshape(2, LN) / 7.0
    x = np.linspace(0.1, 0.6, LN)
    a0, w0, a1, w1 = [0.3, -0.2], [1.5, 0.5], [0.7], [2.0]
    # rank 1 alone, to record what it contributes to each of rank 0's four all-reduces
    s1 = OpenStubShard(a1, w1, LN)
    s1.forward(x)
    sums1 = s1.sums()
    f_tot = complex(StubShard(a0, w0, LN).sums()[0] + sums1[0], StubShard(a0, w0, LN).sums()[1] + sums1[1])
    _, ds1 = s1.open_hvp_forward(V)
    ds0 = StubShard(a0, w0, LN).hvp_forward(V)[1]
    hv1 = s1.open_hvp_backward(f_tot, ds0 + ds1)
    other = [sums1, s1.backward(f_tot), ds1.view(np.float64), hv1]
    s0 = OpenStubShard(a0, w0, LN)
    ev = ShardedEvaluator(s0, 3, 0, dist=SumOfShards(other))
    with pytest.raises(RuntimeError, match="eval_host first"):
        ev.hvp_host(V)
    ev.eval_host(x)
    HV = ev.hvp_host(V)
    assert s0.calls == ["forward", "backward", "open_hvp_forward", "open_hvp_backward"]
    assert s0.got[0] == f_tot                                   # the all-reduced f of the evaluation, kept from eval_host
    assert np.array_equal(s0.got[1], ds0 + ds1)                 # the all-reduced f'
    want = f_tot.imag * np.real(ds0 + ds1)[:, None] * np.ones(LN) * 2 + (sum(a0) + sum(a1)) * V
    assert HV.shape == (2, LN) and np.abs(HV - want).max() <= 1e-14
    # a single process: no collective, the handle's own sums
    s = OpenStubShard(a0, w0, LN)
    ev = ShardedEvaluator(s, 2, 0)
    ev.eval_host(x)
    HV = ev.hvp_host(V)
    assert s.calls == ["forward", "backward", "open_hvp_forward", "open_hvp_backward"]
    assert s.got[0] == complex(s.sums()[0], s.sums()[1]) and np.array_equal(s.got[1], ds0)
