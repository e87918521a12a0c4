"""grape_open_hvp (csrc/grape_lindblad_hvp.hip.h) -- what can be checked without a GPU: the entry points through every layer
(header, export list, ctypes binding, Julia glue), the refusals that come before the first HIP call, the shape checks of the
Python method, and the resource usage of the eight instantiations of the kernels."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_open_host import _create, _tiny  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    from grape_jl_amd import api
    header = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert re.search(r"^int grape_open_hvp\(grape_handle \*h, int nv, const double \*V, double \*HV\);", header, re.M)
    assert re.search(r"^int grape_get_open_hvp_info\(grape_handle \*h, double \*out, int n\);", header, re.M)
    assert "#define GRAPE_HIP_ABI_VERSION 7" in header                  # entry points only
    assert "grape_open_hvp" in api.EXPORTS and "grape_get_open_hvp_info" in api.EXPORTS
    assert callable(api.GrapeHipOpen.open_hvp) and callable(api.GrapeHipOpen.open_hvp_info)
    assert api.GrapeHipOpen.hvp is api.GrapeHip.hvp              # the inherited method stays grape_hvp: its refusal is defined
    julia = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    assert "function open_hvp!(HV::VecOrMat{Float64}, h::Handle, V::VecOrMat{Float64})" in julia
    assert "ccall((:grape_open_hvp, libgrape), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64})" in julia
    assert "function open_hvp_info(h::Handle)" in julia
    assert "ccall((:grape_get_open_hvp_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint)" in julia


def test_null_arguments_are_refused_with_a_message():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    lib = api.load_library()
    assert lib.grape_open_hvp.argtypes == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert lib.grape_get_open_hvp_info.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    v, out = np.zeros(3), np.zeros(7)
    assert lib.grape_open_hvp(None, 1, v.ctypes.data, out.ctypes.data) == -1
    assert b"grape_open_hvp: h == NULL" in lib.grape_last_error(None)
    assert lib.grape_open_hvp(None, 0, None, None) == -1
    assert lib.grape_get_open_hvp_info(None, out.ctypes.data, 7) == -1
    # with a handle (where a device exists): the argument checks and "no evaluation yet"; the handle is still there to destroy
    p, d, keep = _tiny(api)
    rc, h, msg = _create(lib, p, d)
    assert rc in (0, -2), (rc, msg)
    if rc == 0:
        for nv, pv, po in ((0, v.ctypes.data, out.ctypes.data), (1, None, out.ctypes.data), (1, v.ctypes.data, None)):
            assert lib.grape_open_hvp(h, nv, pv, po) == -1
            assert b"nv must be positive, V and HV must not be NULL" in lib.grape_last_error(h)
        assert lib.grape_open_hvp(h, 1, v.ctypes.data, out.ctypes.data) == -1
        assert b"no evaluation" in lib.grape_last_error(h)
        assert lib.grape_get_open_hvp_info(h, out.ctypes.data, 7) == 7 and not out.any()
        lib.grape_destroy(h)


def test_the_python_method_checks_the_shape_of_V():
    """before any call into the library: an instance without a handle is enough"""
    from grape_jl_amd import api
    h = api.GrapeHipOpen.__new__(api.GrapeHipOpen)
    h.L, h.N_T, h._h = 2, 3, None
    for bad in (np.zeros(5), np.zeros((2, 5)), np.zeros((0, 6)), np.zeros((1, 2, 3)), np.zeros(())):
        with pytest.raises(ValueError, match=r"V must be \[L\*N_T\] = \[6\]"):
            h.open_hvp(bad)


def test_new_header_is_a_build_source():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_lindblad_hvp.hip.h") in srcs
    main = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_lindblad_hvp.hip.h"' in main
    old = open(os.path.join(api._CSRC, "grape_lindblad.hip.h")).read()
    assert "hvp" not in old                                              # the set of kernels there does not change


def test_hvp_kernels_have_no_scratch(tmp_path):
    """All eight instantiations (forward and backward, NP = 16 ... 64) keep their matrices in the workspace and their running sums
    in registers (forward) or in the workspace (backward): no scratch (private memory) on gfx950, within the registers their
    workgroup sizes leave (16 waves at NP = 64 forward: 128 per lane; 9 waves at NP = 48 backward: 168; 8 at NP = 64: 256)."""
    src = tmp_path / "lind_hvp.hip"
    inst = "".join(f"template __global__ void lind_hvp_{kind}_kernel<{np_}>(LindHvpArgs);\n"
                   for kind in ("forward", "backward") for np_ in (16, 32, 48, 64))
    src.write_text('#include "grape_lindblad_hvp.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "lind_hvp.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for b in res.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_Z2\dlind_hvp_(forward|backward)_kernelILi(\d+)EEv11LindHvpArgs", b)
        if not m:
            continue
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)]
        vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", b)]
        assert scratch == [0], b[:1500]
        seen[(m.group(1), int(m.group(2)))] = vgprs[0]
    print(dict(vgprs=seen))
    assert sorted(seen) == [(kind, np_) for kind in ("backward", "forward") for np_ in (16, 32, 48, 64)], res.stderr[-2000:]
    assert seen[("forward", 64)] <= 128 and seen[("backward", 48)] <= 168 and seen[("backward", 64)] <= 256
