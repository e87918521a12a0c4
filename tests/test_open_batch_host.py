"""grape_open_eval_batch (csrc/grape_lindblad_batch.hip.h) -- what can be checked without a GPU: the entry points through every
layer (header, export list, ctypes binding, Julia glue), the refusals that come before the first HIP call, the shape check of
the Python method, and the resource usage of the eight instantiations of the kernels."""
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
    assert re.search(r"^int grape_open_eval_batch\(grape_handle \*h, int P, const double \*pulsevals, double \*J, double \*G, "
                     r"double \*tau\);", header, re.M)
    assert re.search(r"^int grape_get_open_batch_info\(grape_handle \*h, double \*out, int n\);", header, re.M)
    assert "#define GRAPE_HIP_ABI_VERSION 7" in header                  # entry points only
    assert "grape_open_eval_batch" in api.EXPORTS and "grape_get_open_batch_info" in api.EXPORTS
    assert callable(api.GrapeHipOpen.open_eval_batch) and callable(api.GrapeHipOpen.open_batch_info)
    assert api.GrapeHipOpen.eval_batch is api.GrapeHip.eval_batch   # the inherited method stays grape_eval_batch: the loop route
    julia = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    assert ("function open_eval_batch!(h::Handle, J::Vector{Float64}, G::Union{Nothing,Matrix{Float64}}, "
            "tau::Union{Nothing,Matrix{ComplexF64}},") in julia
    assert "ccall((:grape_open_eval_batch, libgrape), Cint," in julia
    assert "GrapeHIP.open_eval_batch!: handles with pseudo-controls" in julia
    assert "function open_batch_info(h::Handle)" in julia
    assert "ccall((:grape_get_open_batch_info, libgrape), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint)" in julia


def test_null_arguments_are_refused_with_a_message():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    lib = api.load_library()
    vp = ctypes.c_void_p
    assert lib.grape_open_eval_batch.argtypes == [vp, ctypes.c_int, vp, vp, vp, vp]
    assert lib.grape_get_open_batch_info.argtypes == [vp, vp, ctypes.c_int]
    x, out = np.zeros(3), np.zeros(7)
    assert lib.grape_open_eval_batch(None, 1, x.ctypes.data, out.ctypes.data, None, None) == -1
    assert lib.grape_last_error(None) == b"grape_open_eval_batch: h == NULL"
    assert lib.grape_open_eval_batch(None, 0, None, None, None, None) == -1
    assert lib.grape_get_open_batch_info(None, out.ctypes.data, 7) == -1
    # with a handle (where a device exists): the argument checks; the handle is still there to destroy
    p, d, keep = _tiny(api)
    rc, h, msg = _create(lib, p, d)
    assert rc in (0, -2), (rc, msg)
    if rc == 0:
        for P, px, pj, needle in ((0, x.ctypes.data, out.ctypes.data, b"P must be positive"),
                                  (1, None, out.ctypes.data, b"pulsevals == NULL"), (1, x.ctypes.data, None, b"J == NULL")):
            assert lib.grape_open_eval_batch(h, P, px, pj, None, None) == -1
            assert needle in lib.grape_last_error(h)
        assert lib.grape_get_open_batch_info(h, out.ctypes.data, 7) == 7 and not out.any()
        lib.grape_destroy(h)


def test_the_python_method_checks_the_shape_of_pulsevals():
    """before any call into the library: an instance without a handle is enough"""
    from grape_jl_amd import api
    h = api.GrapeHipOpen.__new__(api.GrapeHipOpen)
    h.L, h.N_T, h.K, h._h = 2, 3, 1, None
    for bad in (np.zeros(6), np.zeros((2, 5)), np.zeros((1, 2, 3)), np.zeros(())):
        with pytest.raises(ValueError, match=r"pulsevals must be \[P, L\*N_T\] = \[P, 6\]"):
            h.open_eval_batch(bad)


def test_new_header_is_a_build_source():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_lindblad_batch.hip.h") in srcs
    main = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_lindblad_batch.hip.h"' in main
    units = [f for f in os.listdir(api._CSRC) if f.endswith(".hip")]
    assert sorted(units) == ["grape_hip.hip", "grape_t18.hip"]           # no new translation unit


def test_batch_kernels_have_no_scratch_and_use_the_f64_mfma(tmp_path):
    """All eight instantiations (forward and backward, NP = 16 ... 64) keep their matrices in the workspace of their set and
    their running sums in registers (forward) or in the workspace (backward): no scratch (private memory) on gfx950, within
    the registers their workgroup sizes leave (16 waves at NP = 64 forward: 128 per lane; 9 waves at NP = 48 backward: 168; 8
    at NP = 64: 256).  The NP = 64 forward kernel multiplies on v_mfma_f64_16x16x4."""
    src = tmp_path / "lind_batch.hip"
    inst = "".join(f"template __global__ void lind_batch_{kind}_kernel<{np_}>(LindArgs, LindBatchStrides);\n"
                   for kind in ("forward", "backward") for np_ in (16, 32, 48, 64))
    src.write_text('#include "grape_lindblad_batch.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-save-temps",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "lind_batch.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for b in res.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_Z2\dlind_batch_(forward|backward)_kernelILi(\d+)EEv8LindArgs16LindBatchStrides", b)
        if not m:
            continue
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)]
        vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", b)]
        assert scratch == [0], b[:1500]
        seen[(m.group(1), int(m.group(2)))] = vgprs[0]
    print(dict(vgprs=seen))
    assert sorted(seen) == [(kind, np_) for kind in ("backward", "forward") for np_ in (16, 32, 48, 64)], res.stderr[-2000:]
    assert seen[("forward", 64)] <= 128 and seen[("backward", 48)] <= 168 and seen[("backward", 64)] <= 256
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s")]
    assert len(asm) == 1, asm
    text = open(tmp_path / asm[0]).read()
    start = text.index("_Z25lind_batch_forward_kernelILi64EEv8LindArgs16LindBatchStrides:")
    body = text[start:text.index("s_endpgm", start)]
    assert body.count("v_mfma_f64_16x16x4") >= 16, body.count("v_mfma_f64_16x16x4")
