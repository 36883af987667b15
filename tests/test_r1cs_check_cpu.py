"""CPU: the witness check against an R1CS (zkr_r1cs_load / _check / _check_device / _matches_key) refuses null arguments and a
malformed r1cs_bin without touching a device -- with the messages of the one parser the setups use -- and its kernels keep no
stack frame (the compiler-metadata check test_kernel_resources.py makes for the proving path)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
HIPCC = "/opt/rocm/bin/hipcc"
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _u32(x):
    return int(x).to_bytes(4, "little")


def _side(terms):
    return _u32(len(terms)) + b"".join(_u32(s) + int(cf).to_bytes(32, "little") for s, cf in terms)


def _system(n_vars, n_public, rows):
    return _u32(n_vars) + _u32(n_public) + _u32(len(rows)) + b"".join(_side(a) + _side(b) + _side(c) for a, b, c in rows)


GOOD = _system(3, 1, [([(1, 1)], [(1, 1)], [(2, 1)]), ([(2, 5)], [(0, 1)], [])])


def test_null_arguments_are_argument_errors():
    import zkr_hip
    L = zkr_hip.lib()
    out, ok = ctypes.c_void_p(), ctypes.c_int(7)
    rep = (ctypes.c_uint64 * 3)()
    info = (ctypes.c_uint64 * 6)()
    ptrs = (ctypes.c_void_p * 1)(ctypes.c_void_p(0))
    hosts = (ctypes.c_char_p * 1)(b"\0" * 96)
    handle = ctypes.c_void_p(8)      # never dereferenced: every call below fails its argument check first
    assert L.zkr_r1cs_load(None, 0, 0, ctypes.byref(out)) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_r1cs_load(GOOD, len(GOOD), 0, None) == -5
    assert L.zkr_r1cs_info(None, info) == -5 and L.zkr_r1cs_info(handle, None) == -5
    assert L.zkr_r1cs_check_device(None, ptrs, 1, None, rep, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_check_device(handle, None, 1, None, rep, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_check_device(handle, ptrs, 1, None, rep, None) == -5
    assert L.zkr_r1cs_check_device(handle, ptrs, 0, None, rep, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_check_device(handle, ptrs, 1, None, rep, ctypes.byref(ok)) == -5     # a null witness pointer in the list
    assert L.zkr_r1cs_check(None, hosts, 96, 1, rep, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_check(handle, None, 96, 1, rep, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_check(handle, hosts, 96, 1, rep, None) == -5
    assert L.zkr_r1cs_check(handle, hosts, 96, 0, rep, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_matches_key(None, handle, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_matches_key(handle, None, ctypes.byref(ok)) == -5
    assert L.zkr_r1cs_matches_key(handle, handle, None) == -5
    L.zkr_r1cs_free(None)            # as free(NULL)


@pytest.mark.parametrize("name,buf,needle", [
    ("shorter than its header", GOOD[:11], "R1CS shorter than its header"),
    ("truncated in a constraint", GOOD[:12 + 40 + 40 + 20], "R1CS truncated in constraint 0"),
    ("truncated between the sides", GOOD[:12 + 40 + 40 + 40 + 40], "R1CS truncated in constraint 1"),
    ("a signal >= nVars", _system(3, 1, [([(3, 1)], [(1, 1)], [(2, 1)])]), "constraint 0: signal 3 out of range or coefficient >= r"),
    ("a coefficient >= r", _system(3, 1, [([(1, 1)], [(1, R)], [(2, 1)])]), "constraint 0: signal 1 out of range or coefficient >= r"),
    ("trailing bytes", GOOD + b"\0\0", "R1CS has 2 trailing bytes"),
])
def test_malformed_systems_are_refused_by_the_parser_before_any_device_call(name, buf, needle):
    import zkr_hip
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.ConstraintSystem.load(buf)
    assert e.value.code == -5 and needle in str(e.value), name
    with pytest.raises(zkr_hip.ZkrError) as e2:     # the one parser: the setup refuses the same buffer with the same words
        zkr_hip.ProvingKey.setup_r1cs(buf, toxic=[2, 3, 4, 5, 6])
    assert e2.value.code == -5 and needle in str(e2.value), name


def test_a_well_formed_system_without_a_device_is_no_device():
    import zkr_hip
    if zkr_hip.device_count() > 0:
        cs = zkr_hip.ConstraintSystem.load(GOOD)
        assert cs.info() == {"nVars": 3, "nPublic": 1, "nConstraints": 2, "nnzA": 2, "nnzB": 2, "nnzC": 1}
        cs.close()
        return
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.ConstraintSystem.load(GOOD)
    assert e.value.code == -1 and "no CPU fallback" in str(e.value)


def test_python_host_exposes_the_check():
    import zkr_hip
    for name in ("load", "info", "check", "check_device", "matches_key", "close"):
        assert callable(getattr(zkr_hip.ConstraintSystem, name)), name
    with pytest.raises(ValueError):
        zkr_hip.ConstraintSystem(None, 0).check([b"\0" * 64, b"\0" * 32])     # ragged witnesses never reach the C side


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_r1cs_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "zkr_r1cs.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
                           "--cuda-device-only", "-S", os.path.join(PKG, "csrc", "zkr_r1cs.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    rows = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        rows[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2)).group(1))
    own = [k for k in rows if "r1cs_" in k]
    assert len(own) == 3   # check, check_wide, match
    assert any("spmv_kernel" in k for k in rows) and any("spmv_wide_kernel" in k for k in rows)   # the key's own row kernels, for matches_key
    assert {k: v for k, v in rows.items() if v} == {}
