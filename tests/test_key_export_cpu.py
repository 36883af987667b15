"""CPU: the export of a device key as websnark bytes -- its entry points exist and check their arguments before any device call,
the format's arithmetic (zkr_websnark_len) and writer (zkr_websnark_render_host) reproduce the oracle's key byte for byte, the
writer passes its sanitizer build in a program of its own, the export kernels keep no stack frame, and the Node host declares
its three calls."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256


def _mont(v):
    return (v * MONT % R).to_bytes(32, "little")


def _csr(pols, m):
    """polsA / polsB as the oracle holds them ({constraint: coefficient} per signal) -> (rowptr, col, coefs) by row, Montgomery"""
    rows = [[] for _ in range(m)]
    for sig, d in enumerate(pols):
        for c, v in d.items():
            rows[c].append((sig, v))
    rowptr, col, coef = [0], [], []
    for r in rows:
        for sig, v in r:
            col.append(sig)
            coef.append(_mont(v))
        rowptr.append(len(col))
    return rowptr, col, b"".join(coef)


def _sections(pkb):
    n, p, m = struct.unpack_from("<3I", pkb, 0)
    ptr = list(struct.unpack_from("<7I", pkb, 12)) + [len(pkb)]
    return n, p, m, ptr, [pkb[ptr[2 + t]:ptr[3 + t]] for t in range(5)]


def test_symbols_resolve_and_arguments_are_checked_before_the_device():
    import zkr_hip
    from zkr_hip import binding
    L = zkr_hip.lib()
    for name in ("zkr_key_export_websnark", "zkr_websnark_len", "zkr_websnark_render_host"):
        assert hasattr(L, name), name
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.zkr_key_export_websnark(None, None, ctypes.byref(out), ctypes.byref(n)) == -5 and b"null" in L.zkr_last_error()
    fake = ctypes.c_void_p(0)
    assert L.zkr_key_export_websnark(fake, None, None, None) == -5 and b"null" in L.zkr_last_error()
    # an unknown flag is refused before the key is looked at: the null handle is never read
    opts = binding.KeyExportOpts(2, 0)
    assert L.zkr_key_export_websnark(None, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(n)) == -5 and b"unknown export flag" in L.zkr_last_error()
    opts = binding.KeyExportOpts(binding.EXPORT_STANDARD | 0x80, 0)
    assert L.zkr_key_export_websnark(None, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(n)) == -5 and b"unknown export flag 0x80" in L.zkr_last_error()
    assert out.value is None
    assert L.zkr_websnark_len(4, 1, 4, 1, 1, None) == -5
    pts = (ctypes.c_char_p * 5)()
    assert L.zkr_websnark_render_host(4, 1, 4, None, None, None, None, None, None, None, pts, ctypes.byref(out), ctypes.byref(n)) == -5


def test_websnark_len_is_the_oracle_keys_length_and_refuses_what_the_format_cannot_hold(small_case):
    import zkr_hip
    pk = small_case["pk"]
    nnz_a = sum(len(d) for d in pk["polsA"])
    nnz_b = sum(len(d) for d in pk["polsB"])
    assert zkr_hip.websnark_len(pk["nVars"], pk["nPublic"], pk["domainSize"], nnz_a, nnz_b) == len(small_case["pkb"])
    # a 2^23 key with two terms per row and side: 384 B of points per signal alone are 3.2 GB
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.websnark_len(1 << 23, 73, 1 << 23, 2 << 23, 2 << 23)
    assert e.value.code == -5 and "limited to 4 GiB" in str(e.value)
    assert zkr_hip.websnark_len(1 << 22, 73, 1 << 22, 2 << 22, 2 << 22) == 488 + (8 + 72 + 72 + 64 * 4 + 128) * (1 << 22) - 64 * 74
    for bad in ((0, 0, 4, 0, 0), (4, 4, 4, 0, 0), (4, 1, 6, 0, 0), (4, 1, 1 << 33, 0, 0)):
        with pytest.raises(zkr_hip.ZkrError):
            zkr_hip.websnark_len(*bad)


def test_render_host_reproduces_the_oracle_key(small_case):
    import zkr_hip
    pk, pkb = small_case["pk"], small_case["pkb"]
    n, p, m, ptr, pts = _sections(pkb)
    assert (n, p, m) == (pk["nVars"], pk["nPublic"], pk["domainSize"])
    got = zkr_hip.websnark_render_host(n, p, m, pkb[40:488], _csr(pk["polsA"], m), _csr(pk["polsB"], m), pts)
    assert got == pkb


def test_render_host_keeps_duplicates_and_zero_coefficients_in_their_stored_order():
    """Signal 1 has two terms in row 2 (7, then 5: not merged into 12, not swapped) and a zero coefficient in row 0; signal 0's
    list crosses rows out of CSR position; signal 2 has no term on side A."""
    import zkr_hip
    n, p, m = 3, 0, 4
    # side A by row: row 0: (sig 1, 0) (sig 0, 9); row 1: -; row 2: (sig 1, 7) (sig 0, 4) (sig 1, 5); row 3: (sig 0, 1)
    a = ([0, 2, 2, 5, 6], [1, 0, 1, 0, 1, 0], b"".join(_mont(v) for v in (0, 9, 7, 4, 5, 1)))
    b = ([0, 0, 1, 1, 1], [2], _mont(3))
    consts = bytes(range(256)) + bytes(range(192))
    pts = [bytes([0x10 + t]) * (k * sz) for t, (k, sz) in enumerate(((n, 64), (n, 64), (n, 128), (n - p - 1, 64), (m, 64)))]
    got = zkr_hip.websnark_render_host(n, p, m, consts, a, b, pts)
    u32 = lambda v: struct.pack("<I", v)
    lst = lambda terms: u32(len(terms)) + b"".join(u32(c) + _mont(v) for c, v in terms)
    pols_a = lst([(0, 9), (2, 4), (3, 1)]) + lst([(0, 0), (2, 7), (2, 5)]) + lst([])
    pols_b = lst([]) + lst([]) + lst([(1, 3)])
    ptrs, off = [], 488
    for blob in [pols_a, pols_b] + pts:
        ptrs.append(off)
        off += len(blob)
    want = u32(n) + u32(p) + u32(m) + b"".join(u32(x) for x in ptrs) + consts + pols_a + pols_b + b"".join(pts)
    assert got == want
    assert zkr_hip.websnark_len(n, p, m, 6, 1) == len(want)
    # rows that do not ascend, a signal that is none of the key's: refused, nothing returned
    for bad_a in (([0, 2, 1, 5, 6], a[1], a[2]), ([1, 2, 2, 5, 6], a[1], a[2]), (a[0], [1, 0, 3, 0, 1, 0], a[2])):
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.websnark_render_host(n, p, m, consts, bad_a, b, pts)
        assert e.value.code == -5


def test_key_export_selfcheck_under_sanitizers():
    """`make key-export-asan`: csrc/key_export_selfcheck.cpp, a plain executable over websnark_writer.cpp built with AddressSanitizer
    and UBSan -- nothing is preloaded, no Python and no HIP in that process."""
    r = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "key-export-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "key_export_selfcheck: ok" in r.stdout


def test_export_kernels_have_no_private_segment():
    """tools/kernel_resources.py on the new unit (the compiler's own metadata): both kernels, neither with scratch -- the point
    moves in 16-byte pieces and is converted where it lands, by calls that take a pointer (curve29.hpp radix_to_256_at)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "zkr_key_export", "--all-kernels"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    head = re.search(r"== zkr_key_export\.hip: (\d+) kernels, (\d+) with scratch", r.stdout)
    assert head and int(head.group(1)) == 2 and int(head.group(2)) == 0, r.stdout
    rows = re.findall(r"scratch\s+(\d+) B\s+vgpr\+agpr\s+(\d+).*?(export_points_kernel<\w+\s*>)", r.stdout)
    assert len(rows) == 2 and all(int(s) == 0 for s, _, _ in rows), r.stdout


def test_node_host_declares_its_three_calls():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert re.search(r"\bexportKey\(opts\?: KeyExportOptions\): ArrayBuffer", dts)
    assert re.search(r"\bexportKeyJson\(\): ProvingKeyJson", dts)
    assert re.search(r"export function keyToWebsnark\(key: KeyHandle, opts\?: KeyExportOptions\): ArrayBuffer", dts)
    js = open(os.path.join(PKG, "index.js")).read()
    for name in ("exportKey", "exportKeyJson", "keyToWebsnark"):
        assert name in js, name
