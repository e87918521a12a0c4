"""grape_hvp_forward / grape_hvp_backward / grape_hvp_backward_chi (csrc/grape_hvp_split.hip.h) -- what can be
checked without a GPU: the entry points through every layer (header, export list, ctypes binding, Julia glue), the refusals
that come before the first HIP call, the shape checks of the Python methods, the resource usage of the eight instantiations
of the new sweep kernel, and the protocol of ShardedEvaluator.hvp_host on stub handles."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = (r"int grape_hvp_forward\(grape_handle \*h, int nv, const double \*V, double \*dtau, double \*dsums, double \*dpsiT\);",
         r"int grape_hvp_backward\(grape_handle \*h, int nv, const double f_total\[2\], const double \*df_total, double \*HV\);",
         r"int grape_hvp_backward_chi\(grape_handle \*h, int nv, const double \*chi, const double \*dchi, double \*HV\);")
NAMES = ("grape_hvp_forward", "grape_hvp_backward", "grape_hvp_backward_chi")


def test_entry_points_are_declared_exported_bound_and_called_from_julia():
    from grape_jl_amd import api
    header = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    for d in DECLS:
        assert re.search("^" + d, header, re.M), d
    assert "#define GRAPE_HIP_ABI_VERSION 7" in header                  # entry points only
    for n in NAMES:
        assert n in api.EXPORTS
    for m in ("hvp_forward", "hvp_backward", "hvp_backward_chi"):
        assert callable(getattr(api.GrapeHip, m))
    julia = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for fn in ("function hvp_forward!(h::Handle, V::VecOrMat{Float64};", "function hvp_backward!(HV::VecOrMat{Float64}, h::Handle,",
               "function hvp_backward_chi!(HV::VecOrMat{Float64}, h::Handle,"):
        assert fn in julia, fn
    for n in NAMES:
        assert "ccall((:%s, libgrape), Cint" % n in julia, n


def _tiny_problem(api):
    N, K, L, N_T = 4, 1, 1, 3
    keep = dict(tlist=np.linspace(0.0, 1.0, N_T + 1), H0=np.zeros((K, N, N), complex), Hc=np.zeros((L, N, N), complex),
                psi0=np.ones((K, N), complex), target=np.ones((K, N), complex))
    p = api._Problem()
    p.abi_version, p.N, p.K, p.K_total, p.N_T, p.L = api.ABI_VERSION, N, K, K, N_T, L
    for name, arr in keep.items():
        setattr(p, name, arr.ctypes.data)
    return p, keep


def test_null_arguments_are_refused_with_a_message():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    lib = api.load_library()
    vp, ip = ctypes.c_void_p, ctypes.c_int
    assert lib.grape_hvp_forward.argtypes == [vp, ip, vp, vp, vp, vp]
    assert lib.grape_hvp_backward.argtypes == [vp, ip, vp, vp, vp]
    assert lib.grape_hvp_backward_chi.argtypes == [vp, ip, vp, vp, vp]
    a = np.zeros(64)
    d = a.ctypes.data
    assert lib.grape_hvp_forward(None, 1, d, None, None, None) == -1
    assert b"grape_hvp_forward: h == NULL" in lib.grape_last_error(None)
    assert lib.grape_hvp_backward(None, 1, d, d, d) == -1
    assert b"grape_hvp_backward: h == NULL" in lib.grape_last_error(None)
    assert lib.grape_hvp_backward_chi(None, 1, d, d, d) == -1
    assert b"grape_hvp_backward_chi: h == NULL" in lib.grape_last_error(None)
    # with a handle (where a device exists): the argument checks, then "nothing evaluated" / "no forward half"
    p, keep = _tiny_problem(api)
    h = ctypes.c_void_p()
    rc = lib.grape_create(ctypes.byref(h), ctypes.byref(p))
    assert rc in (0, -2), (rc, lib.grape_last_error(None))
    if rc == 0:
        for nv, v in ((0, d), (1, None)):
            assert lib.grape_hvp_forward(h, nv, v, None, None, None) == -1
            assert b"grape_hvp_forward: nv must be positive, V must not be NULL" in lib.grape_last_error(h)
        for args in ((0, d, d, d), (1, None, d, d), (1, d, None, d), (1, d, d, None)):
            assert lib.grape_hvp_backward(h, *args) == -1
            assert b"grape_hvp_backward: nv must be positive, f_total, df_total and HV must not be NULL" in lib.grape_last_error(h)
            assert lib.grape_hvp_backward_chi(h, *args) == -1
            assert b"grape_hvp_backward_chi: nv must be positive, chi, dchi and HV must not be NULL" in lib.grape_last_error(h)
        assert lib.grape_hvp_forward(h, 1, d, None, None, None) == -1
        assert b"grape_hvp_forward: no valid forward state" in lib.grape_last_error(h)
        assert lib.grape_hvp_backward(h, 1, d, d, d) == -1
        assert b"grape_hvp_backward: no grape_hvp_forward on this handle yet" in lib.grape_last_error(h)
        assert lib.grape_hvp_backward_chi(h, 1, d, d, d) == -1
        assert b"grape_hvp_backward_chi: no grape_hvp_forward on this handle yet" in lib.grape_last_error(h)
        lib.grape_destroy(h)
    _ = keep


def _bare():
    """an instance without a handle: the shape checks come before any call into the library"""
    from grape_jl_amd import api
    h = api.GrapeHip.__new__(api.GrapeHip)
    h.L, h.N_T, h.K, h.N, h._h = 2, 3, 2, 4, None
    return h


def test_the_python_methods_check_their_shapes():
    h = _bare()
    for bad in (np.zeros(5), np.zeros((2, 5)), np.zeros((0, 6)), np.zeros((1, 2, 3)), np.zeros(())):
        with pytest.raises(ValueError, match=r"V must be \[L\*N_T\] = \[6\]"):
            h.hvp_forward(bad)
    for bad in (np.zeros((2, 2), complex), np.zeros(0, complex)):
        with pytest.raises(ValueError, match="df_total must be"):
            h.hvp_backward(1.0 + 0j, bad)
    chi = np.zeros((2, 4), complex)
    with pytest.raises(ValueError, match=r"chi must be \[K, N\] = \[2, 4\]"):
        h.hvp_backward_chi(np.zeros((2, 5), complex), chi)
    for bad in (np.zeros((2, 5), complex), np.zeros((3, 2, 5), complex), np.zeros((0, 2, 4), complex), np.zeros(8, complex),
                np.zeros((1, 1, 2, 4), complex)):
        with pytest.raises(ValueError, match="dchi must be"):
            h.hvp_backward_chi(chi, bad)


def test_new_header_is_a_build_source_and_the_old_one_is_untouched():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_hvp_split.hip.h") in srcs
    main = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_hvp_split.hip.h"' in main
    old = open(os.path.join(api._CSRC, "grape_hvp.hip.h")).read()
    assert "split" not in old and "chi_kernel" not in old          # the set of kernels there does not change


def test_backward_chi_kernels_have_no_scratch(tmp_path):
    """All eight instantiations of hvp_backward_chi_kernel (NP = 16 ... 64, one and two column tiles) keep the running sums in
    registers and the term block in the LDS, as hvp_backward_kernel does: no scratch (private memory) on gfx950, at most 35 KB
    of LDS, within the 256 registers per lane at which a SIMD still holds two waves (512 per lane on gfx950).  Measured: 92 ... 108
    VGPRs with one column tile, 137 ... 140 with two (204 at NP = 16, where one wave owns every row)."""
    src = tmp_path / "hvp_split.hip"
    inst = "".join(f"template __global__ void hvp_backward_chi_kernel<{np_}, {nct}>(HvpArgs, const double2 *, const double2 *);\n"
                   for np_ in (16, 32, 48, 64) for nct in (1, 2))
    src.write_text('#include "grape_hvp_split.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "hvp_split.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for b in res.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_Z23hvp_backward_chi_kernelILi(\d+)ELi(\d)EEv7HvpArgs", b)
        if not m:
            continue
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)]
        vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", b)]
        lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", b)]
        assert scratch == [0], b[:1500]
        assert lds and lds[0] <= 35 * 1024, b[:1500]
        seen[(int(m.group(1)), int(m.group(2)))] = (vgprs[0], lds[0])
    print(dict(vgprs_lds=seen))
    assert sorted(seen) == [(np_, nct) for np_ in (16, 32, 48, 64) for nct in (1, 2)], res.stderr[-2000:]
    assert all(v <= 256 for v, _ in seen.values())


class StubShard:
    """a handle of K local trajectories whose 'H v' depends on everything that crosses the reductions, so that a wrong or
    missing all-reduce shows: tau'_k = (1 + 2i) a_k sum(V_j),  H v_j = Im f_total Re f'_total,j + (sum_k a_k) V_j"""
    def __init__(self, a, w, LN):
        self.a, self._weights, self.LN, self.calls = np.asarray(a, float), np.asarray(w, float), LN, []

    def forward(self, x):
        self.calls.append("forward")
        return self.a * np.sum(x) + 0j

    def sums(self):
        f = np.sum(self._weights * self.a)
        return np.array([f, 0.5 * f, 0.0, f, 0.0, 0.0, 0.0, 0.0])

    def backward(self, f_total):
        self.calls.append("backward")
        return np.full(self.LN, complex(f_total).real)

    def hvp_forward(self, V):
        self.calls.append("hvp_forward")
        self.V = np.asarray(V, float)
        dtau = self.a[None, :] * self.V.sum(axis=-1, keepdims=True) * (1 + 2j)
        return dtau, (dtau * self._weights[None, :]).sum(axis=1)

    def hvp_backward(self, f_total, df_total):
        self.calls.append("hvp_backward")
        self.got = (complex(f_total), np.array(df_total))
        return complex(f_total).imag * np.real(df_total)[:, None] * np.ones(self.LN) + self.a.sum() * self.V


class SumOfShards:
    """torch.distributed stand-in for ONE rank of two: all_reduce adds the other rank's recorded contribution"""
    def __init__(self, other):
        self.other, self.n = other, 0

    def all_reduce(self, t):
        import torch
        t += torch.from_numpy(np.array(self.other[self.n], dtype=np.float64))
        self.n += 1


def test_sharded_hvp_host_on_stub_handles():
    from grape_jl_amd.sharded import ShardedEvaluator
    LN = 6
    V = np.arange(12.0).reshape(2, LN) / 7.0
    x = np.linspace(0.1, 0.6, LN)
    a0, w0, a1, w1 = [0.3, -0.2], [1.5, 0.5], [0.7], [2.0]
    # rank 1 alone, to record what it contributes to each of rank 0's four all-reduces
    s1 = StubShard(a1, w1, LN)
    s1.forward(x)
    sums1 = s1.sums()
    f_tot = complex(StubShard(a0, w0, LN).sums()[0] + sums1[0], StubShard(a0, w0, LN).sums()[1] + sums1[1])
    _, ds1 = s1.hvp_forward(V)
    ds0 = StubShard(a0, w0, LN).hvp_forward(V)[1]
    hv1 = s1.hvp_backward(f_tot, ds0 + ds1)
    other = [sums1, s1.backward(f_tot), ds1.view(np.float64), hv1]
    s0 = StubShard(a0, w0, LN)
    ev = ShardedEvaluator(s0, 3, 0, dist=SumOfShards(other))
    with pytest.raises(RuntimeError, match="eval_host first"):
        ev.hvp_host(V)
    ev.eval_host(x)
    HV = ev.hvp_host(V)
    assert s0.calls == ["forward", "backward", "hvp_forward", "hvp_backward"]
    assert s0.got[0] == f_tot                                   # the all-reduced f of the evaluation, kept from eval_host
    assert np.array_equal(s0.got[1], ds0 + ds1)                 # the all-reduced f'
    want = f_tot.imag * np.real(ds0 + ds1)[:, None] * np.ones(LN) * 2 + (sum(a0) + sum(a1)) * V
    assert HV.shape == (2, LN) and np.abs(HV - want).max() <= 1e-14
    # a single process: no collective, the handle's own sums
    s = StubShard(a0, w0, LN)
    ev = ShardedEvaluator(s, 2, 0)
    ev.eval_host(x)
    HV = ev.hvp_host(V)
    assert s.got[0] == complex(s.sums()[0], s.sums()[1]) and np.array_equal(s.got[1], ds0)
