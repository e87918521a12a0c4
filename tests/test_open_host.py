"""Open-system handles (grape_create_open, csrc/grape_lindblad.hip.h) -- what can be checked without a GPU: the argument
validation (before the first HIP call), the host helper ``liouvillian`` against the Lindblad equation written out in matrix
form, and the resource usage of the new kernels."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_helpers as oh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(api, N=4, K=1, L=1, N_T=3, J=1):
    keep = dict(tlist=np.linspace(0.0, 1.0, N_T + 1), H0=np.zeros((K, N, N), complex), Hc=np.zeros((L, N, N), complex),
                psi0=np.ones((K, N, N), complex), target=np.ones((K, N, N), complex))
    p = api._Problem()
    p.abi_version, p.N, p.K, p.K_total, p.N_T, p.L = api.ABI_VERSION, N, K, K, N_T, L
    for name, arr in keep.items():
        setattr(p, name, arr.ctypes.data)
    keep["cops"] = np.zeros((max(J, 1), N, N), complex)
    d = api._Lindblad()
    d.J, d.cops_per_traj, d.cops = J, 0, keep["cops"].ctypes.data
    return p, d, keep


def _create(lib, p, d):
    h = ctypes.c_void_p()
    rc = lib.grape_create_open(ctypes.byref(h), ctypes.byref(p), None if d is None else ctypes.byref(d))
    return rc, h, lib.grape_last_error(None)


def test_create_open_refusals_come_before_the_first_hip_call():
    import __graft_entry__ as entry
    entry.build()
    from grape_jl_amd import api
    lib = api.load_library()
    cases = []

    def case(reason, needle, **kw):
        p, d, keep = _tiny(api, **{k: v for k, v in kw.items() if k in ("N", "J")})
        cases.append((reason, needle, p, d, keep, kw))

    case("N > 64", b"N > 64", N=65)
    case("J < 0", b"J < 0", J=-1)
    case("J > 8", b"J > 8", J=9)
    case("cops == NULL with J > 0", b"cops == NULL", cops_null=True)
    case("diss == NULL", b"diss == NULL", diss_null=True)
    case("gradient_method", b"GRAPE_GRAD_GRADGEN", gradient_method=api.GRAD_TAYLOR)
    case("prop_method", b"GRAPE_PROP_EXP", prop_method=api.PROP_SERIES)
    case("Dpen", b"Dpen", dpen=True)
    case("ndev > 1", b"ndev > 1", ndev=2)
    for reason, needle, p, d, keep, kw in cases:
        if kw.get("cops_null"):
            d.cops = None
        if "gradient_method" in kw:
            p.gradient_method = kw["gradient_method"]
        if "prop_method" in kw:
            p.prop_method = kw["prop_method"]
        if kw.get("dpen"):
            keep["D"] = np.zeros((p.N, p.N), complex)
            p.Dpen = keep["D"].ctypes.data
        if "ndev" in kw:
            p.ndev = kw["ndev"]
        rc, h, msg = _create(lib, p, None if kw.get("diss_null") else d)
        assert rc == -1, (reason, rc, msg)
        assert not h.value, reason
        assert needle in msg, (reason, msg)
    # the checks shared with grape_create
    p, d, keep = _tiny(api)
    p.abi_version = 99
    assert _create(lib, p, d)[0] == -1
    p, d, keep = _tiny(api, L=1)
    p.L = 0
    assert _create(lib, p, d)[0] == -6
    # J = 0 with cops = NULL is unitary evolution of a density matrix: it gets as far as the device
    p, d, keep = _tiny(api, J=0)
    d.cops = None
    rc, h, msg = _create(lib, p, d)
    assert rc in (0, -2), (rc, msg)
    if rc == 0:
        lib.grape_destroy(h)
    # target == NULL stays legal, exactly as on the closed path
    p, d, keep = _tiny(api)
    p.target = None
    rc, h, msg = _create(lib, p, d)
    assert rc in (0, -2), (rc, msg)
    if rc == 0:
        lib.grape_destroy(h)


def _random_case(rng, d=3, J=2, hermitian=False):
    H = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    if hermitian:
        H = H + H.conj().T
    cops = [0.4 * (rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))) for _ in range(J)]
    rho = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    return H, cops, rho


@pytest.mark.parametrize("hermitian", [False, True])
def test_liouvillian_is_the_lindblad_equation_in_vectorised_form(hermitian):
    from grape_jl_amd import liouvillian
    rng = np.random.default_rng(5)
    H, cops, rho = _random_case(rng, hermitian=hermitian)
    Lv = liouvillian(H, cops)
    want = oh.vec(oh.lindblad_rhs(H, cops, rho))
    got = -1j * Lv @ oh.vec(rho)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # the same matrix as the tests' own construction, and linear in H (the control part is liouvillian(H_l))
    assert np.abs(Lv - oh.super_generator(H, cops)).max() <= 1e-14 * np.abs(Lv).max()
    H2 = rng.normal(size=H.shape) + 0j
    assert np.abs(liouvillian(H + 0.3 * H2, cops) - Lv - 0.3 * liouvillian(H2)).max() <= 1e-14 * np.abs(Lv).max()


def test_liouvillian_keeps_the_trace_for_hermitian_generators():
    import scipy.linalg
    from grape_jl_amd import liouvillian
    rng = np.random.default_rng(6)
    H, cops, X = _random_case(rng, hermitian=True)
    rho = X @ X.conj().T
    rho /= np.trace(rho)
    for t in (0.1, 1.0, 3.0):
        v = scipy.linalg.expm(-1j * liouvillian(H, cops) * t) @ oh.vec(rho)
        rt = v.reshape(3, 3).T   # un-stack the columns
        assert abs(np.trace(rt) - 1.0) <= 1e-13
        assert np.abs(rt - rt.conj().T).max() <= 1e-13


def test_new_kernels_have_no_scratch_and_use_the_f64_mfma(tmp_path):
    """Every instantiation of the two Lindblad kernels keeps its state in registers and in its workspace: no scratch
    (private memory) on gfx950; the NP = 64 forward kernel multiplies on v_mfma_f64_16x16x4."""
    src = tmp_path / "lind.hip"
    inst = "".join(f"template __global__ void lind_{w}_kernel<{np_}>(LindArgs);\n"
                   for w in ("forward", "backward") for np_ in (16, 32, 48, 64))
    src.write_text('#include "grape_lindblad.hip.h"\n' + inst)
    res = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-save-temps",
                          "-I", os.path.join(ROOT, "grape.jl_amd", "csrc"), "-Rpass-analysis=kernel-resource-usage",
                          str(src), "-o", str(tmp_path / "lind.o")], capture_output=True, text=True, cwd=tmp_path)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = 0
    for b in res.stderr.split("Function Name: ")[1:]:
        if "lind_" not in b.splitlines()[0]:
            continue
        seen += 1
        scratch = [re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln) for ln in b.splitlines()]
        scratch = [int(m.group(1)) for m in scratch if m]
        assert scratch == [0], b[:1500]
    assert seen == 8, res.stderr[-2000:]
    asm = [f for f in os.listdir(tmp_path) if f.endswith(".s")]
    assert len(asm) == 1, asm
    text = open(tmp_path / asm[0]).read()
    start = text.index("_Z19lind_forward_kernelILi64EEv8LindArgs:")
    body = text[start:text.index("s_endpgm", start)]
    assert body.count("v_mfma_f64_16x16x4") >= 16, body.count("v_mfma_f64_16x16x4")


def test_new_header_is_a_build_source():
    from grape_jl_amd import api
    srcs, _ = api._sources()
    assert os.path.join(api._CSRC, "grape_lindblad.hip.h") in srcs
    assert "grape_create_open" in api.EXPORTS


def test_synthetic_open_problem_is_physical():
    from grape_jl_amd import synth
    pr = synth.make_open_config("O8K8")
    assert pr["cops"].shape == (2, 8, 8) and pr["rho0"].shape == (8, 8, 8)
    for rho in list(pr["rho0"]) + list(pr["target"]):
        assert abs(np.trace(rho) - 1.0) < 1e-14 and np.abs(rho - rho.conj().T).max() < 1e-15
        assert np.linalg.eigvalsh(rho).min() > 0.0
