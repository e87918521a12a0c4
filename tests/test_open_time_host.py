"""grape_open_time_gradient (csrc/grape_lindblad_tg.hip.h) -- what can be checked without a GPU: the entry point through every
layer (header, export list, ctypes binding, Julia glue), the refusals that come before the first HIP call, and the resource
usage of the four instantiations of the kernel."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_open_host import _create, _tiny  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    from grape_jl_amd import api
    header = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    assert re.search(r"^int grape_open_time_gradient\(grape_handle \*h, double \*dJdt", header, re.M)
    assert "#define GRAPE_HIP_ABI_VERSION 7" in header                  # an entry point only
    assert "grape_open_time_gradient" in api.EXPORTS
    assert hasattr(api.GrapeHipOpen, "time_gradient") and api.GrapeHipOpen.time_gradient is not api.GrapeHip.time_gradient
    julia = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    assert "function open_time_gradient!(dJdt::Vector{Float64}, h::Handle)" in julia
    assert "ccall((:grape_open_time_gradient, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64})" in julia


def test_null_arguments_are_refused_with_a_message():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    lib = api.load_library()
    assert lib.grape_open_time_gradient.argtypes == [ctypes.c_void_p, ctypes.c_void_p]
    out = np.zeros(3)
    assert lib.grape_open_time_gradient(None, out.ctypes.data) == -1
    assert b"grape_open_time_gradient: h == NULL" in lib.grape_last_error(None)
    assert lib.grape_open_time_gradient(None, None) == -1
    # with a handle (where a device exists): dJdt == NULL, and "no evaluation yet"; the handle is still there to destroy
    p, d, keep = _tiny(api)
    rc, h, msg = _create(lib, p, d)
    assert rc in (0, -2), (rc, msg)
    if rc == 0:
        assert lib.grape_open_time_gradient(h, None) == -1
        assert b"dJdt == NULL" in lib.grape_last_error(h)
        assert lib.grape_open_time_gradient(h, out.ctypes.data) == -1
        assert b"no evaluation" in lib.grape_last_error(h)
        lib.grape_destroy(h)


def test_new_header_is_a_build_source():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_lindblad_tg.hip.h") in srcs
    main = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_lindblad_tg.hip.h"' in main


def test_time_gradient_kernel_has_no_scratch(tmp_path):
    """Every instantiation keeps the running sum of the chi chain in registers and everything else in its workspace: no
    scratch (private memory) on gfx950, also at NP = 64 with 16 waves and 128 registers per lane."""
    src = tmp_path / "lind_tg.hip"
    inst = "".join(f"template __global__ void lind_timegrad_kernel<{np_}>(LindArgs);\n" for np_ in (16, 32, 48, 64))
    src.write_text('#include "grape_lindblad_tg.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "lind_tg.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for b in res.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_Z20lind_timegrad_kernelILi(\d+)EEv8LindArgs", b)
        if not m:
            continue
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)]
        vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", b)]
        assert scratch == [0], b[:1500]
        seen[int(m.group(1))] = vgprs[0]
    print(dict(vgprs=seen))
    assert sorted(seen) == [16, 32, 48, 64], res.stderr[-2000:]
    assert seen[64] <= 128          # 16 waves of 64 lanes on a CU
