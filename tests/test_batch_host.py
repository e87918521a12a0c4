"""grape_eval_batch / grape_get_batch_info without a GPU: the entry points exist in the header, the library, the ctypes binding
and the Julia glue, the ABI version did not move, and a NULL handle is refused before anything touches HIP."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grape_eval_batch", "grape_get_batch_info")


def _header():
    return open(os.path.join(ROOT, "include", "grape_hip.h")).read()


def test_entry_points_are_declared_exported_bound_and_called_from_julia():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+grape_eval_batch\s*\(\s*grape_handle\s*\*\s*h\s*,\s*int\s+P\s*,\s*const\s+double\s*\*\s*pulsevals\s*,"
                     r"\s*double\s*\*\s*J\s*,\s*double\s*\*\s*G\s*,\s*double\s*\*\s*tau\s*\)\s*;", code)
    assert re.search(r"int\s+grape_get_batch_info\s*\(\s*grape_handle\s*\*\s*h\s*,\s*double\s*\*\s*out\s*,\s*int\s+n\s*\)\s*;", code)
    lib = ctypes.CDLL(api.library_path())
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert re.search(r"ccall\(\(:" + name + r",\s*libgrape\)", jl), name
    assert "function eval_batch!(" in jl and "function batch_info(" in jl
    assert hasattr(api.GrapeHip, "eval_batch") and hasattr(api.GrapeHip, "batch_info")


def test_the_abi_version_did_not_move():
    from grape_jl_amd import api
    assert re.search(r"#define\s+GRAPE_HIP_ABI_VERSION\s+7\b", _header())
    assert api.ABI_VERSION == 7
    assert re.search(r"^const ABI_VERSION = 7\s*$", open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read(), flags=re.M)
    lib = api.load_library()
    assert lib.grape_abi_version() == 7


def test_null_handle_is_refused_without_touching_hip():
    import numpy as np
    from grape_jl_amd import api
    lib = api.load_library()
    x, J, out = np.zeros(4), np.zeros(1), np.full(4, 7.0)
    assert lib.grape_eval_batch(None, 1, x.ctypes.data, J.ctypes.data, None, None) == -1
    assert lib.grape_get_batch_info(None, out.ctypes.data, 4) == -1
    assert (out == 7.0).all() and J[0] == 0.0


def test_the_new_header_rebuilds_the_library():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert any(os.path.basename(s) == "grape_batch.hip.h" for s in srcs)
    assert os.path.exists(os.path.join(ROOT, "grape.jl_amd", "csrc", "grape_batch.hip.h"))
