"""csrc/grape_devmem.h -- the tracked allocator of the handles and the grow-only storage of a launch group -- without a GPU:
a stand-alone program (tests/devmem_driver.cpp) that defines the HIP calls of the header over malloc / free, built by the host
compiler under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devmem_header_is_a_build_source_and_no_translation_unit():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_devmem.h") in srcs
    assert '#include "grape_devmem.h"' in open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    text = open(os.path.join(api._CSRC, "grape_devmem.h")).read()
    assert "__global__" not in text and "__device__" not in text and "hip_runtime.h" not in text      # host only


def test_devmem_under_address_and_ub_sanitizers(tmp_path):
    """release twice, aliased pointers, a failure at every position of a layout, grow-only, the budget rule clause by clause,
    skipped zero-sized requests (see the driver); any report of a sanitizer aborts the binary"""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    exe = str(tmp_path / "devmem_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), os.path.join(ROOT, "tests", "devmem_driver.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "devmem-driver OK" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
