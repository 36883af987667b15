"""CPU: what the operator step (include/zkr.h zkr_operator_*, zkr_hip.rollup.Operator, index.js Ledger / Operator / txRow) promises
without a device: the symbols, the refusals that come before any device call, the blinding check in Python, the Node row codec
against Python's, the Node ledger's loud failure without a GPU, and the type declarations."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
NODE = shutil.which("node")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(PKG, "napi", "zkr_napi.node")),
                                reason="node or the N-API addon is not available")
SYMBOLS = ("zkr_operator_new", "zkr_operator_free", "zkr_operator_info", "zkr_operator_step", "zkr_operator_stage_times")


def _node(script, *args):
    r = subprocess.run([NODE, "-e", script, *args], cwd=PKG, capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        raise AssertionError(r.stderr)
    return r.stdout


def test_operator_symbols_are_declared_exported_and_bound():
    import zkr_hip
    import zkr_hip.binding as b
    L = zkr_hip.lib()
    header = open(os.path.join(ROOT, "include", "zkr.h")).read()
    binding = open(b.__file__).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), "libzkr_hip.so does not export %s" % name
        assert "L.%s.argtypes" % name in binding, name
    assert ctypes.sizeof(b.OperatorOpts) == 16


def test_null_arguments_are_refused_before_any_device_call():
    import zkr_hip
    from zkr_hip.binding import OperatorOpts
    L = zkr_hip.lib()
    out, opts = ctypes.c_void_p(), OperatorOpts(2, 0, 0, 0)
    fake = ctypes.c_void_p(8)                     # never dereferenced: a null neighbour is found first
    assert L.zkr_operator_new(None, fake, None, None, ctypes.byref(opts), ctypes.byref(out)) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_operator_new(fake, None, None, None, ctypes.byref(opts), ctypes.byref(out)) == -5
    assert L.zkr_operator_new(fake, fake, None, None, None, ctypes.byref(out)) == -5
    assert L.zkr_operator_new(fake, fake, None, None, ctypes.byref(opts), None) == -5
    assert not out.value
    u64, dbl, sz = (ctypes.c_uint64 * 6)(), (ctypes.c_double * 6)(), ctypes.c_size_t()
    assert L.zkr_operator_info(None, u64) == -5 and L.zkr_operator_info(fake, None) == -5
    assert L.zkr_operator_stage_times(None, dbl) == -5 and L.zkr_operator_stage_times(fake, None) == -5
    buf = ctypes.create_string_buffer(256)
    assert L.zkr_operator_step(None, buf, 1, None, None, buf, buf, buf, ctypes.byref(sz), ctypes.byref(sz)) == -5
    assert L.zkr_operator_step(fake, buf, 1, None, None, buf, buf, buf, None, ctypes.byref(sz)) == -5
    assert L.zkr_operator_step(fake, buf, 1, None, None, buf, buf, buf, ctypes.byref(sz), None) == -5
    assert L.zkr_operator_step(fake, None, 1, None, None, buf, buf, buf, ctypes.byref(sz), ctypes.byref(sz)) == -5
    assert L.zkr_operator_step(fake, buf, 1, None, None, None, buf, buf, ctypes.byref(sz), ctypes.byref(sz)) == -5
    assert b"null" in L.zkr_last_error()
    L.zkr_operator_free(None)                     # as free(NULL)


def test_step_refuses_a_short_blinding_list_before_the_library_is_called():
    """The C side reads 32 bytes of r and of s per batch the queue can fill: a shorter list must not reach it.  The operator here has
    no handle at all, so a call that got as far as the library would fail in another way."""
    from zkr_hip import rollup as n
    op = n.Operator.__new__(n.Operator)
    op._h, op._held, op.batch, op.n_public = None, None, 2, 49
    rows = [[1, 2, 3, 4, 5, 6, 7, 8]] * 4         # two batches
    for rs, ss in (([1], [1]), ([1, 2], [1]), ([1, 2, 3], [1, 2, 3]), ([1, 2], None), (None, [1, 2])):
        with pytest.raises(ValueError):
            op.step(rows, rs, ss)


@needs_node
def test_node_tx_row_bytes_equal_pythons():
    from zkr_hip import rollup as n
    top = (1 << 250) - 1                          # 250-bit values: every byte of a word but the last carries bits
    vals = [top, top - 2, top - 12345, top >> 1, top - (1 << 200), top - 7, (1 << 250) - (1 << 249) + 99, top - 1]
    sig = {"R8": (vals[5], vals[6]), "S": vals[7]}
    want = b"".join(int(v).to_bytes(32, "little") for v in n.tx_row(vals[0], vals[1], vals[2], vals[3], vals[4], sig))
    out = _node("""
      const z = require('./index.js');
      const v = JSON.parse(process.argv[1]).map(BigInt);
      const row = z.txRow(v[0], v[1].toString(), v[2], v[3], v[4].toString(), { R8: [v[5], v[6].toString()], S: v[7] });
      console.log(JSON.stringify({ hex: Buffer.from(row).toString('hex'), small: Buffer.from(z.txRow(1, 2, 3, 4, 5, { R8: [6, 7], S: 8 })).toString('hex') }));
    """, json.dumps([str(v) for v in vals]))
    got = json.loads(out)
    assert len(want) == 256 and bytes.fromhex(got["hex"]) == want
    assert bytes.fromhex(got["small"]) == b"".join(int(v).to_bytes(32, "little") for v in range(1, 9))


@needs_node
def test_node_ledger_fails_loudly_without_its_device():
    out = _node("""
      const z = require('./index.js');
      const absent = z.deviceCount();
      let msg = null;
      try { new z.Ledger(3, absent); } catch (e) { msg = e.message; }
      let restored = null;
      try { z.Ledger.restore(Buffer.alloc(64), absent); } catch (e) { restored = e.message; }
      console.log(JSON.stringify({ absent, msg, restored, classes: [typeof z.Ledger, typeof z.Operator, typeof z.txRow] }));
    """)
    got = json.loads(out)
    assert got["msg"] is not None and "no HIP device %d" % got["absent"] in got["msg"] and "no CPU fallback" in got["msg"]
    assert got["restored"] is not None                     # a blob that is no snapshot is refused on the host
    assert got["classes"] == ["function", "function", "function"]


def test_type_declarations_carry_the_new_surface():
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert re.search(r"export class Ledger\b", dts) and re.search(r"export class Operator\b", dts)
    assert re.search(r"export function txRow\(", dts)
    for method in ("deposit(", "root()", "account(", "info()", "snapshot()", "static restore(", "save(", "static load(", "checkpoint()", "rollback(",
                   "release(", "journalInfo()", "close()", "step(", "stageTimes()"):
        assert method in dts, method
