"""csrc/grape_evalstate.h -- the one record of what the last evaluation left on the device, its events and its queries -- without
a GPU: a stand-alone program (tests/evalstate_driver.cpp) that walks every sequence of at most six events against a model and
holds every refusal a caller can read against the sentences of the library before the record existed, built by the host
compiler under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evalstate_header_is_a_build_source_plain_cxx_and_the_only_state_word():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_evalstate.h") in srcs                  # (a change of the header rebuilds the library)
    main = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_evalstate.h"' in main
    text = open(os.path.join(api._CSRC, "grape_evalstate.h")).read()
    assert "__global__" not in text and "__device__" not in text and not re.search(r"#include\s*[<\"][^>\"]*hip", text)   # no HIP at all
    # the words the record replaced are gone from the library's host code
    for word in ("tg_state", "hv_state", "ex_state", "have_bwd", "tg_unit", "tg_xi_user", "tg_chi_user", "came(", "OPEN_TG_REFUSE"):
        assert word not in main, word
    assert not re.search(r"\b(TG|HV)_[A-Z]+\b", main)
    assert main.count("StoredEval ev;") == 1                                      # one record per handle, open handles included


def test_evalstate_under_address_and_ub_sanitizers(tmp_path):
    """every event sequence up to length six on a closed and on an open record, the sentence table (see the driver); any report
    of a sanitizer aborts the binary.  No HIP include path, no HIP definitions: the header is plain C++17."""
    exe = str(tmp_path / "evalstate_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), os.path.join(ROOT, "tests", "evalstate_driver.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "evalstate-driver OK" in res.stdout and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
