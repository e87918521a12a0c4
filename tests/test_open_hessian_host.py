"""grape_open_hessian / grape_get_open_hessian_info without a GPU: the entry points exist in the header, the library, the
ctypes binding and the Julia glue, the ABI version did not move, a NULL handle is refused before anything touches HIP,
``GrapeHipOpen.open_hessian`` shapes its result, and no instantiation of the new kernels uses scratch memory."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grape_open_hessian", "grape_get_open_hessian_info")
KERNELS = ("lind_hess_forward_seeds_kernel", "lind_hess_theta_kernel", "lind_hess_backward_seeds_kernel", "lind_hess_fan_kernel")


def _header():
    return open(os.path.join(ROOT, "include", "grape_hip.h")).read()


def test_entry_points_are_declared_exported_bound_and_called_from_julia():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+grape_open_hessian\s*\(\s*grape_handle\s*\*\s*h\s*,\s*double\s*\*\s*H\s*\)\s*;", code)
    assert re.search(r"int\s+grape_get_open_hessian_info\s*\(\s*grape_handle\s*\*\s*h\s*,\s*double\s*\*\s*out\s*,\s*int\s+n\s*\)\s*;", code)
    assert re.search(r"#define\s+GRAPE_HIP_ABI_VERSION\s+7\b", _header()) and api.ABI_VERSION == 7
    lib = ctypes.CDLL(api.library_path())
    assert lib.grape_abi_version() == 7
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert re.search(r"ccall\(\(:" + name + r",\s*libgrape\)", jl), name
    assert "function open_hessian!(" in jl and "function open_hessian_info(" in jl
    assert hasattr(api.GrapeHipOpen, "open_hessian") and hasattr(api.GrapeHipOpen, "open_hessian_info")
    srcs, _ = api._sources()
    assert any(os.path.basename(s) == "grape_lindblad_hessian.hip.h" for s in srcs)    # (a change of the new header rebuilds the library)
    main = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_lindblad_hessian.hip.h"' in main


def test_null_handle_is_refused_without_touching_hip():
    """(a NULL H needs a handle, and a handle a device: tests/test_gpu_open_hessian.py refuses it there)"""
    from grape_jl_amd import api
    lib = api.load_library()
    H, out = np.full(4, 7.0), np.full(12, 7.0)
    assert lib.grape_open_hessian(None, H.ctypes.data) == -1 and lib.grape_open_hessian(None, None) == -1
    assert lib.grape_last_error(None).startswith(b"grape_open_hessian:")
    assert lib.grape_get_open_hessian_info(None, out.ctypes.data, 12) == -1
    assert (H == 7.0).all() and (out == 7.0).all()


class _FakeLib:
    """stands in for the C library behind GrapeHipOpen.open_hessian: fills H with its flat index, the info with 1..12"""

    def __init__(self, P):
        self.P, self.calls = P, 0

    def grape_open_hessian(self, h, outptr):
        out = np.ctypeslib.as_array(ctypes.cast(outptr, ctypes.POINTER(ctypes.c_double)), shape=(self.P * self.P,))
        out[:] = np.arange(self.P * self.P)
        self.calls += 1
        return 0

    def grape_get_open_hessian_info(self, h, outptr, n):
        out = np.ctypeslib.as_array(ctypes.cast(outptr, ctypes.POINTER(ctypes.c_double)), shape=(n,))
        out[:] = np.arange(1, n + 1)
        return n


def test_shape_handling_of_open_hessian():
    from grape_jl_amd import api
    h = api.GrapeHipOpen.__new__(api.GrapeHipOpen)          # no handle, no device: only the argument handling is exercised
    h.L, h.N_T, h._h = 2, 3, None
    h._lib = _FakeLib(6)
    H = h.open_hessian()
    assert H.shape == (6, 6) and H.dtype == np.float64 and H.flags["C_CONTIGUOUS"]
    assert np.array_equal(H, np.arange(36.0).reshape(6, 6))
    assert h._lib.calls == 1
    info = h.open_hessian_info()
    assert info == dict(series_terms=1, series_steps=2, traj_per_pass=3, bytes=4, ms=5.0, terms_forward_seeds=6,
                        terms_backward_seeds=7, terms_fan=8, steps_forward_seeds=9, steps_backward_seeds=10, steps_fan=11,
                        fan_columns=12)


def test_no_instantiation_of_the_new_kernels_uses_scratch(tmp_path):
    """Every NP = 16 / 32 / 48 / 64 instantiation keeps its chains in registers or in its workspace: no scratch (private memory)
    on gfx950, and the 16-wave kernels of NP = 64 fit the 128 registers per lane that 16 waves on a compute unit leave."""
    src = tmp_path / "lind_hess.hip"
    inst = "".join(f"template __global__ void {k}<{np_}>(LindHessArgs);\n" for k in KERNELS for np_ in (16, 32, 48, 64))
    src.write_text('#include "grape_lindblad_hessian.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "lind_hess.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for b in res.stderr.split("Function Name: ")[1:]:
        m = re.match(r"_Z\d+(lind_hess_\w+_kernel)ILi(\d+)EEv12LindHessArgs", b)
        if not m:
            continue
        scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", b)]
        vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", b)]
        assert scratch == [0], b[:1500]
        seen[(m.group(1), int(m.group(2)))] = vgprs[0]
    print(dict(vgprs=seen))
    assert sorted(seen) == sorted((k, np_) for k in KERNELS for np_ in (16, 32, 48, 64)), res.stderr[-2000:]
    for k in ("lind_hess_forward_seeds_kernel", "lind_hess_theta_kernel", "lind_hess_fan_kernel"):
        assert seen[(k, 64)] <= 128                                                                              # 16 waves of 64 lanes
    assert seen[("lind_hess_backward_seeds_kernel", 64)] <= 256                                                  # 8 waves
