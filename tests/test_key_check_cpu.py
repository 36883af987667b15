"""CPU: the key-content check (zkr_key_check) is exported, refuses a null key without touching a device, is declared in every
host, and its kernels keep no stack frame (the same compiler-metadata check test_kernel_resources.py makes for the proving path)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
HIPCC = "/opt/rocm/bin/hipcc"
SECTIONS = ("NONE", "ROWPTR", "COL", "WIDE", "RANK", "HEADER", "POINTS", "TWIDDLES", "COEF", "SHARED_RANK", "CONSTS")


def test_null_key_is_an_argument_error():
    import zkr_hip
    L = zkr_hip.lib()
    assert L.zkr_key_check(None, 0, None) == -5
    assert b"null" in L.zkr_last_error()
    rep = (ctypes.c_uint64 * 4)()
    assert L.zkr_key_check(None, 1, rep) == -5


def test_sections_are_named_in_the_header_in_report_order():
    src = open(os.path.join(ROOT, "include", "zkr.h")).read()
    for i, name in enumerate(SECTIONS):
        assert re.search(r"\bZKR_KEYSEC_%s = %d\b" % (name, i), src), name
    assert re.search(r"int zkr_key_check\(const zkr_key \*key, int level, uint64_t report\[4\]\);", src)


def test_python_and_node_hosts_expose_the_check():
    import zkr_hip
    from zkr_hip import binding
    assert binding.KEY_SECTIONS == tuple(s.lower().replace("_", " ") for s in SECTIONS)
    assert callable(zkr_hip.ProvingKey.check)
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert re.search(r"\bcheckKey\(opts\?: \{ deep\?: boolean \}\)", dts)
    assert "checkKey(opts)" in open(os.path.join(PKG, "index.js")).read()
    napi = open(os.path.join(PKG, "napi", "zkr_napi.c")).read()
    assert '"zkr_key_check"' in napi and '{"keyCheck"' in napi


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_key_check_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "zkr_key_check.s"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
                           "--cuda-device-only", "-S", os.path.join(PKG, "csrc", "zkr_key_check.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    rows = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        rows[m.group(1)] = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", m.group(2)).group(1))
    checks = [k for k in rows if "_check_kernel" in k]
    assert len(checks) == 6   # csr, rank, coef, twiddle, points<Fq>, points<Fq2>
    assert {k: v for k, v in rows.items() if v} == {}
