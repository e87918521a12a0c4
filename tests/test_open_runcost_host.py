"""State running costs on open-system handles (grape_open_set_running_cost, grape_open_backward_xi,
csrc/grape_lindblad_rc.hip.h) -- what can be checked without a GPU: the exports, the build sources, the refusal of a NULL
handle (before the first HIP call) and the resource usage of the new backward kernel."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("grape_open_set_running_cost", "grape_open_backward_xi")


def test_exports_and_header_name_the_two_calls():
    """(tests/test_abi.py compares the two lists; this pins the names)"""
    from grape_jl_amd import api
    header = open(os.path.join(ROOT, "include", "grape_hip.h")).read()
    for name in NAMES:
        assert name in api.EXPORTS
        assert re.search(r"\bint " + name + r"\(grape_handle \*h,", header), name
    assert api.ABI_VERSION == 7 and "#define GRAPE_HIP_ABI_VERSION 7" in header


def test_new_header_is_a_build_source():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_lindblad_rc.hip.h") in srcs
    assert os.path.exists(os.path.join(api._CSRC, "grape_lindblad_rc.hip.h"))


def test_a_null_handle_is_refused_with_a_message():
    import numpy as np
    import grape_jl_amd as g
    from grape_jl_amd import api
    g.build_library()
    lib = api.load_library()
    p = np.zeros(4).ctypes.data
    assert lib.grape_open_set_running_cost(None, p, 0, 0.5) == -1
    assert b"grape_open_set_running_cost" in lib.grape_last_error(None) and b"NULL" in lib.grape_last_error(None)
    assert lib.grape_open_backward_xi(None, p, None, p, 0.5, p) == -1
    assert b"grape_open_backward_xi" in lib.grape_last_error(None) and b"NULL" in lib.grape_last_error(None)


def test_the_backward_kernel_with_a_running_cost_has_no_scratch(tmp_path):
    """every instantiation of lind_backward_rc_kernel keeps its state in registers and in its workspace, as the kernel it
    restates does (tests/test_open_host.py): no scratch (private memory) on gfx950"""
    src = tmp_path / "lind_rc.hip"
    inst = "".join(f"template __global__ void lind_backward_rc_kernel<{np_}>(LindArgs, LindRcArgs);\n" for np_ in (16, 32, 48, 64))
    src.write_text('#include "grape_lindblad_rc.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "lind_rc.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = 0
    for b in res.stderr.split("Function Name: ")[1:]:
        if "lind_backward_rc_kernel" not in b.splitlines()[0]:
            continue
        seen += 1
        scratch = [re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln) for ln in b.splitlines()]
        scratch = [int(m.group(1)) for m in scratch if m]
        print(b.splitlines()[0], [ln.strip() for ln in b.splitlines() if "VGPRs:" in ln or "SGPRs Spill" in ln or "Occupancy" in ln])
        assert scratch == [0], b[:1500]
    assert seen == 4, res.stderr[-2000:]
