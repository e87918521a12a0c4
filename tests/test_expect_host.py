"""grape_expect / grape_get_expect_info without a GPU: the entry points exist in the header, the library, the ctypes binding and
the Julia glue, the ABI version did not move, a NULL handle is refused before anything touches HIP, the argument refusals on a
handle (where a device exists), the shape handling of ``GrapeHip.expect`` and the operator layouts of the upload."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grape_expect", "grape_get_expect_info")


def _header():
    return open(os.path.join(ROOT, "include", "grape_hip.h")).read()


def test_entry_points_are_declared_exported_bound_and_called_from_julia():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+grape_expect\s*\(\s*grape_handle\s*\*\s*h\s*,\s*int\s+M\s*,\s*const\s+double\s*\*\s*ops\s*,\s*int\s+ops_per_traj\s*,"
                     r"\s*double\s*\*\s*out\s*\)\s*;", code)
    assert re.search(r"int\s+grape_get_expect_info\s*\(\s*grape_handle\s*\*\s*h\s*,\s*double\s*\*\s*out\s*,\s*int\s+n\s*\)\s*;", code)
    assert re.search(r"#define\s+GRAPE_HIP_ABI_VERSION\s+7\b", _header()) and api.ABI_VERSION == 7
    lib = ctypes.CDLL(api.library_path())
    jl = open(os.path.join(ROOT, "julia", "GrapeHIP.jl")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in api.EXPORTS
        assert re.search(r"ccall\(\(:" + name + r",\s*libgrape\)", jl), name
    assert "function expect!(" in jl and "function expect_info(" in jl
    for cls in (api.GrapeHip, api.GrapeHipOpen):
        assert hasattr(cls, "expect") and hasattr(cls, "expect_info")
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_expect.hip.h") in srcs          # (a change of the new header rebuilds the library)
    host = open(os.path.join(api._CSRC, "grape_hip.hip")).read()
    assert '#include "grape_expect.hip.h"' in host


def _tiny_problem(api):
    N, K, L, N_T = 4, 1, 1, 3
    keep = dict(tlist=np.linspace(0.0, 1.0, N_T + 1), H0=np.zeros((K, N, N), complex), Hc=np.zeros((L, N, N), complex),
                psi0=np.ones((K, N), complex), target=np.ones((K, N), complex))
    p = api._Problem()
    p.abi_version, p.N, p.K, p.K_total, p.N_T, p.L = api.ABI_VERSION, N, K, K, N_T, L
    for name, arr in keep.items():
        setattr(p, name, arr.ctypes.data)
    return p, keep


def test_null_handle_and_bad_arguments_are_refused_without_touching_hip():
    from grape_jl_amd import api
    lib = api.load_library()
    vp, ip = ctypes.c_void_p, ctypes.c_int
    assert lib.grape_expect.argtypes == [vp, ip, vp, ip, vp]
    assert lib.grape_get_expect_info.argtypes == [vp, vp, ip]
    ops, out, info = np.ones(2 * 16), np.full(2 * 4, 7.0), np.full(4, 7.0)
    assert lib.grape_expect(None, 1, ops.ctypes.data, 0, out.ctypes.data) == -1
    assert b"grape_expect: h == NULL" in lib.grape_last_error(None)
    assert lib.grape_get_expect_info(None, info.ctypes.data, 4) == -1
    assert (out == 7.0).all() and (info == 7.0).all()
    # with a handle (where a device exists): the argument checks in the order of the header, then "no evaluation yet"
    p, keep = _tiny_problem(api)
    h = ctypes.c_void_p()
    rc = lib.grape_create(ctypes.byref(h), ctypes.byref(p))
    assert rc in (0, -2), (rc, lib.grape_last_error(None))
    if rc == 0:
        o, r = ops.ctypes.data, out.ctypes.data
        for args, text in (((1, None, 0, r), b"ops == NULL"), ((1, o, 0, None), b"out == NULL"), ((0, o, 0, r), b"M must be positive"),
                           ((-3, o, 0, r), b"M must be positive"), ((17, o, 0, r), b"16"), ((1, o, 2, r), b"ops_per_traj"),
                           ((1, o, -1, r), b"ops_per_traj"), ((1, o, 0, r), b"no evaluation on this handle yet")):
            assert lib.grape_expect(h, *args) == -1, args
            msg = lib.grape_last_error(h)
            assert msg.startswith(b"grape_expect: ") and text in msg, (args, msg)
        assert lib.grape_get_expect_info(h, info.ctypes.data, 4) == 4 and (info == 0.0).all()
        assert lib.grape_get_expect_info(h, None, 4) == -1
        lib.grape_destroy(h)
    assert (out == 7.0).all()
    _ = keep


class _FakeLib:
    """stands in for the C library behind GrapeHip.expect: records the call, returns the (k, n, m) index pattern"""

    def __init__(self):
        self.calls = []

    def grape_expect(self, h, M, optr, per_traj, outptr):
        K, P, N = self.dims
        ops = np.ctypeslib.as_array(ctypes.cast(optr, ctypes.POINTER(ctypes.c_double)), shape=((K if per_traj else 1) * M * N * N * 2,))
        out = np.ctypeslib.as_array(ctypes.cast(outptr, ctypes.POINTER(ctypes.c_double)), shape=(K * P * M * 2,))
        out[:] = np.arange(out.size)
        self.calls.append((M, per_traj, ops.copy()))
        return 0


def test_shape_handling_of_expect():
    from grape_jl_amd import api
    h = api.GrapeHip.__new__(api.GrapeHip)          # no handle, no device: only the argument handling is exercised
    h.K, h.N_T, h.N, h._h = 2, 3, 4, None
    h._lib = _FakeLib()
    h._lib.dims = (2, 4, 4)
    O = (np.arange(3 * 16) + 1j * np.arange(3 * 16)[::-1]).reshape(3, 4, 4)
    out = h.expect(O)
    assert out.shape == (2, 4, 3) and out.dtype == np.complex128 and out[1, 2, 1] == (2 * (1 * 12 + 2 * 3 + 1)) + 1j * (2 * 19 + 1)
    M, per, raw = h._lib.calls[-1]
    assert (M, per) == (3, 0)
    got = (raw[0::2] + 1j * raw[1::2]).reshape(3, 4, 4)
    assert np.array_equal(got, np.swapaxes(O, -1, -2))          # column-major for the ABI: the transpose of numpy's [row, col]
    Ok = np.stack([O, 2 * O])
    out = h.expect(Ok[:, ::-1])                                  # (not contiguous: copied before the pointer is taken)
    M, per, raw = h._lib.calls[-1]
    assert (M, per) == (3, 1) and out.shape == (2, 4, 3)
    assert np.array_equal((raw[0::2] + 1j * raw[1::2]).reshape(2, 3, 4, 4), np.swapaxes(Ok[:, ::-1], -1, -2))
    assert h.expect(np.eye(4)[None]).shape == (2, 4, 1)         # real input
    n = len(h._lib.calls)
    for bad in (np.zeros((4, 4)), np.zeros((3, 4, 5)), np.zeros((3, 5, 5)), np.zeros((3, 2, 4, 4)), np.zeros((1, 2, 3, 4, 4)), 1.0):
        with pytest.raises(ValueError, match="ops must be"):
            h.expect(bad)
    assert len(h._lib.calls) == n


def test_operator_layouts_of_the_upload(tmp_path):
    """expect_pack_closed / expect_pack_open (csrc/grape_expect.hip.h, host code) in a stand-alone program: the fragment order of
    the matrix instruction, the zero padding, the exact congruence D O D and the transposed planar layout of the open kernel"""
    import subprocess
    from grape_jl_amd import api
    src = tmp_path / "pack.cpp"
    src.write_text(r'''
#include <cstdio>
#include <vector>
#include <cstddef>
#define __global__
#define __shared__
#define __device__
#define __forceinline__ inline
''' + _host_part(open(os.path.join(api._CSRC, "grape_expect.hip.h")).read()) + r'''
int main() {
    const int N = 5, NP = 16;
    std::vector<double> O(2 * N * N), bal(N), f(2 * NP * NP, -1.0), w(2 * NP * NP, -1.0);
    for (int j = 0; j < N; ++j) for (int i = 0; i < N; ++i) { O[2 * (j * N + i)] = 10 * i + j; O[2 * (j * N + i) + 1] = -(10 * i + j) - 0.5; }
    for (int i = 0; i < N; ++i) bal[i] = (double)(1 << i);
    expect_pack_closed(O.data(), N, NP, bal.data(), f.data());
    expect_pack_open(O.data(), N, NP, w.data());
    int bad = 0;
    for (int ks = 0; ks < NP / 4; ++ks)
        for (int l = 0; l < 64; ++l) {
            const int i = l & 15, j = 4 * ks + (l >> 4);
            const double s = (i < N && j < N) ? bal[i] * bal[j] : 0.0;
            const double re = (i < N && j < N) ? s * (10 * i + j) : 0.0, im = (i < N && j < N) ? s * (-(10 * i + j) - 0.5) : 0.0;
            if (f[ks * 128 + l] != re || f[ks * 128 + 64 + l] != im) ++bad;
        }
    for (int i = 0; i < NP; ++i)
        for (int j = 0; j < NP; ++j) {
            const bool in = i < N && j < N;   // W[i][j] = O_ji
            if (w[i * NP + j] != (in ? 10 * j + i : 0.0) || w[NP * NP + i * NP + j] != (in ? -(10 * j + i) - 0.5 : 0.0)) ++bad;
        }
    std::printf("%d\n", bad);
    return bad != 0;
}
''')
    exe = tmp_path / "pack"
    subprocess.run(["g++", "-std=c++17", "-O1", str(src), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "0", res.stdout


def _host_part(text):
    """the two packing functions of the header (plain C++ behind the marker comment)"""
    return text[text.index("// ---- host side of the layouts ----"):]
