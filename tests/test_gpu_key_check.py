"""zkr_key_check on the MI355X: every kind of key the library builds passes both levels; an arena whose header is intact but
whose row pointers, columns, wide-row list or rank maps are damaged is refused by zkr_key_load_file, zkr_key_adopt_arena and
zkr_key_adopt_base_arena before any kernel reads through it; a header whose witness tables disagree on the window is refused at
load; value damage passes level 0 and is named by level 1.

Safety: no test proves with, or runs any kernel but the check on, a damaged key.  A damaged load that succeeds is closed at once
and fails the test."""
import ctypes
import os
import shutil
import struct
import subprocess

import pytest

import coracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
T_A, T_B1, T_B2, T_C, T_H = range(5)
TABLES = ("A", "B1", "B2", "C", "H")
RANK_NONE = 0xFFFFFFFF
SPMV_WIDE = 8
FR_MODULUS = 21888242871839275222246405745257275088548364400416034343698204186575808495617

# csrc/zkr_internal.hpp ArenaHeader, field by field (no padding: off_tw lands at byte 64, npts at 40, nnzA at 32)
HDR = struct.Struct("<QQ4I2I5II" "QQ2Q2Q2Q2Q2I5Q5Q" "64s64s64s128s128s" "I5II5I2I2III")
assert HDR.size == 752
WIN_C = struct.calcsize("<QQ4I2I5II" "QQ2Q2Q2Q2Q2I5Q5Q" "64s64s64s128s128s" "I")   # byte offset of win_c[5]


def _header(buf):
    it = iter(HDR.unpack_from(buf, 0))
    take = lambda k: [next(it) for _ in range(k)]
    h = dict(zip(("magic", "total_len", "n", "p", "m", "logm", "nnzA", "nnzB"), take(8)))
    h["npts"], (h["tlog"],) = take(5), take(1)
    h["off_tw"], h["off_twl"] = take(2)
    for f in ("off_rowptr", "off_col", "off_coef", "off_wide", "n_wide"):
        h[f] = take(2)
    h["off_pts"], h["off_rank"] = take(5), take(5)
    h["consts"] = take(5)
    (h["share_b"],), h["win_c"], (h["share_ac"],), h["rank_identity"] = take(1), take(5), take(1), take(5)
    h["sc_lo"], h["sc_n"], h["shard"] = take(2), take(2), take(2)
    h["nnz"] = [h["nnzA"], h["nnzB"]]
    return h


def _u32(buf, off):
    return struct.unpack_from("<I", buf, off)[0]


def _put(off, v):
    return (off, struct.pack("<I", v))


def _entries(h, t):
    return h["sc_n"][1 if t == T_H else 0]


def _rowptr(buf, h, s, i):
    return _u32(buf, h["off_rowptr"][s] + 4 * i)


def _wide_list(buf, h, s):
    return [_u32(buf, h["off_wide"][s] + 4 * j) for j in range(h["n_wide"][s])]


# ---- structural damage: (buf, header) -> [(byte offset, new bytes)], header untouched; (section, part) the check must name
def _col(s):
    def f(buf, h):
        return [_put(h["off_col"][s] + 4 * (h["nnz"][s] // 2), h["n"])]
    return f


def _rowptr_swap(buf, h):
    i = h["m"] // 3
    while not _rowptr(buf, h, 0, i) < _rowptr(buf, h, 0, i + 1):
        i += 1
    assert i + 1 < h["m"]
    return [_put(h["off_rowptr"][0] + 4 * i, _rowptr(buf, h, 0, i + 1)), _put(h["off_rowptr"][0] + 4 * (i + 1), _rowptr(buf, h, 0, i))]


def _rowptr_first(buf, h):
    return [_put(h["off_rowptr"][0], 1)]


def _rowptr_last(buf, h):
    return [_put(h["off_rowptr"][0] + 4 * h["m"], h["nnzA"] - 1)]


def _wide_m(buf, h):
    assert h["n_wide"][1] > 0
    return [_put(h["off_wide"][1], h["m"])]


def _wide_narrow(buf, h):
    wide = _wide_list(buf, h, 1)
    for j in range(1, len(wide) - 1):       # a narrow row between two listed neighbours: the list stays sorted
        for r in range(wide[j - 1] + 1, wide[j + 1]):
            if r != wide[j] and _rowptr(buf, h, 1, r + 1) - _rowptr(buf, h, 1, r) <= SPMV_WIDE:
                return [_put(h["off_wide"][1] + 4 * j, r)]
    raise AssertionError("no narrow row between two wide rows")


def _rank(t):
    def f(buf, h):
        base = h["off_rank"][t]
        i = next(i for i in range(_entries(h, t)) if _u32(buf, base + 4 * i) != RANK_NONE)
        return [_put(base + 4 * i, h["npts"][t])]
    return f


STRUCTURAL = {
    "col_A": (_col(0), "col side A"),
    "col_B": (_col(1), "col side B"),
    "rowptr_swapped": (_rowptr_swap, "rowptr side A"),
    "rowptr_first": (_rowptr_first, "rowptr side A"),
    "rowptr_last": (_rowptr_last, "rowptr side A"),
    "wide_is_m": (_wide_m, "wide side B"),
    "wide_narrow_row": (_wide_narrow, "wide side B"),
}
STRUCTURAL.update({"rank_" + TABLES[t]: (_rank(t), "rank table " + TABLES[t]) for t in range(5)})


def _apply(blob, patches):
    b = bytearray(blob)
    for off, bs in patches:
        b[off:off + len(bs)] = bs
    return bytes(b)


@pytest.fixture(scope="module")
def tx_key(tmp_path_factory):
    """The reference's tx circuit at batch 1, depth 1: wide QAP rows on both sides, non-identity rank maps, every table
    populated; saved once as a packed key file."""
    import zkr_hip
    from zkr_hip import rollup as n
    key, _ = zkr_hip.ProvingKey.setup_r1cs(n.RollupCircuit(1, 1).r1cs(), toxic=[11, 12, 13, 14, 15])
    path = str(tmp_path_factory.mktemp("keycheck") / "tx11.zkrkey")
    key.save(path)
    blob = open(path, "rb").read()
    h = _header(blob)
    assert h["n_wide"][0] > 0 and h["n_wide"][1] > 1 and all(h["npts"])
    assert not all(h["rank_identity"])
    yield dict(key=key, path=path, blob=blob, h=h)
    key.close()


def _refused(load):
    """the damaged load must fail with ZKR_ERR_BAD_KEY; a key it returns anyway is closed unused"""
    import zkr_hip
    try:
        k = load()
    except zkr_hip.ZkrError as e:
        return e
    k.close()
    pytest.fail("a damaged arena was accepted")


def _clone(ptr, nbytes):
    from zkr_hip.batch import _tensor_from_ptr
    return _tensor_from_ptr(ptr, nbytes, 0).clone()


def _patch_tensor(t, patches):
    import torch
    for off, bs in patches:
        t[off:off + len(bs)] = torch.frombuffer(bytearray(bs), dtype=torch.uint8).to(t.device)
    torch.cuda.synchronize()


# ---- 1. valid keys pass both levels
def _clean(key):
    assert key.check(0) == {"bad": 0, "section": "none", "part": 0, "first": 0}
    assert key.check(1) == {"bad": 0, "section": "none", "part": 0, "first": 0}


def test_valid_keys_pass_both_levels(tmp_path, small_case):
    import zkr_hip
    c = small_case
    web = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    _clean(web)
    assert web.prove(c["wb"], c["r"], c["s"]) == coracle.prove(c["pkb"], c["wb"], c["r"], c["s"])   # the check changes no proof
    path = str(tmp_path / "small.zkrkey")
    web.save(path)
    reloaded = zkr_hip.ProvingKey.load_file(path)
    _clean(reloaded)
    assert reloaded.prove(c["wb"], c["r"], c["s"]) == web.prove(c["wb"], c["r"], c["s"])
    for k in (web, reloaded):
        k.close()
    for log_m in (10, 13):
        key, _, _ = zkr_hip.ProvingKey.synth(log_m, want_aux=False)
        _clean(key)
        ptr, n = key.arena()
        mem = _clone(ptr, n)
        replica = zkr_hip.ProvingKey.adopt_arena(mem.data_ptr(), n, 0, keepalive=mem)
        _clean(replica)
        bptr, bn = key.base_arena()
        rebuilt = zkr_hip.ProvingKey.adopt_base_arena(bptr, bn, 0)
        _clean(rebuilt)
        shards = [key.shard(j, 2) for j in range(2)]
        for s in shards:
            _clean(s)
        for k in shards + [rebuilt, replica, key]:
            k.close()


def test_tx_circuit_key_with_wide_rows_passes_both_levels():
    import zkr_hip
    from zkr_hip import rollup as n
    key, _ = zkr_hip.ProvingKey.setup_r1cs(n.RollupCircuit(2, 6).r1cs())
    _clean(key)
    key.close()


# ---- 2. / 3. structural damage is refused on every way in
@pytest.mark.parametrize("case", sorted(STRUCTURAL))
def test_structural_damage_refused_by_load_file(case, tx_key, tmp_path):
    import zkr_hip
    damage, names = STRUCTURAL[case]
    bad = str(tmp_path / "bad.zkrkey")
    with open(bad, "wb") as f:
        f.write(_apply(tx_key["blob"], damage(tx_key["blob"], tx_key["h"])))
    e = _refused(lambda: zkr_hip.ProvingKey.load_file(bad))
    assert e.code == -2 and "key check: " + names + ":" in str(e), str(e)


@pytest.mark.parametrize("case", sorted(STRUCTURAL))
def test_structural_damage_refused_by_adopt_arena(case, tx_key):
    import zkr_hip
    damage, names = STRUCTURAL[case]
    ptr, n = tx_key["key"].arena()
    mem = _clone(ptr, n)
    _patch_tensor(mem, damage(tx_key["blob"], tx_key["h"]))   # the saved file is the arena byte for byte
    e = _refused(lambda: zkr_hip.ProvingKey.adopt_arena(mem.data_ptr(), n, 0, keepalive=mem))
    assert e.code == -2 and "key check: " + names + ":" in str(e), str(e)


@pytest.mark.parametrize("case", sorted(STRUCTURAL))
def test_structural_damage_refused_by_adopt_base_arena(case, tx_key):
    """the compact arena (its own offsets, base points only); rowptr_last -- row_ptr[m] != nnz -- was accepted here before"""
    import zkr_hip
    damage, names = STRUCTURAL[case]
    ptr, n = tx_key["key"].base_arena()
    mem = _clone(ptr, n)
    host = mem.cpu().numpy().tobytes()
    _patch_tensor(mem, damage(host, _header(host)))
    e = _refused(lambda: zkr_hip.ProvingKey.adopt_base_arena(mem.data_ptr(), n, 0))
    assert e.code == -2 and "key check: " + names + ":" in str(e), str(e)


def test_unequal_witness_windows_refused_by_load_file(tmp_path, monkeypatch):
    """A, B1, B2 and C read one set of digit records of w, made with A's window.  c = 17 and c = 18 both give K = 15 window
    levels, so a key file whose B1 window is flipped from 17 to 18 keeps every section offset valid: only that rule refuses it."""
    import zkr_hip
    monkeypatch.setenv("ZKR_MSM_C", "17")   # window bits of keys built in this process
    key, _, _ = zkr_hip.ProvingKey.synth(10, want_aux=False)
    path = str(tmp_path / "c17.zkrkey")
    try:
        key.save(path)
    finally:
        key.close()
    blob = open(path, "rb").read()
    assert _header(blob)["win_c"] == [17] * 5
    bad = str(tmp_path / "bad.zkrkey")
    with open(bad, "wb") as f:
        f.write(_apply(blob, [_put(WIN_C + 4 * T_B1, 18)]))
    e = _refused(lambda: zkr_hip.ProvingKey.load_file(bad))
    assert e.code == -2 and "different windows" in str(e), str(e)


# ---- 4. value damage: level 0 accepts it, level 1 names it
def _flip(off):
    return lambda buf, h: [(off(h), bytes([buf[off(h)] ^ 0x01]))]


def _unshare_b(buf, h):
    assert h["share_b"] and h["npts"][T_B1] == h["npts"][T_B2]
    base = h["off_rank"][T_B2]
    got = _first_b2_entries(h, buf)
    a, b = (_u32(buf, base + 4 * i) for i in got)
    return [_put(base + 4 * got[0], b), _put(base + 4 * got[1], a)]


def _first_b2_entries(h, buf):
    base = h["off_rank"][T_B2]
    return [i for i in range(_entries(h, T_B2)) if _u32(buf, base + 4 * i) != RANK_NONE][:2]


VALUES = {
    # damage, then the report [faulty entries, section, part, first index]: a point of window level 1 of H (levels are stored
    # level-major), a G2 point of B2, a twiddle, a coefficient set to r, B2's rank map made unequal to B1's (two entries swapped:
    # still in range), delta2
    "point_H_level1": (_flip(lambda h: h["off_pts"][T_H] + (h["npts"][T_H] + 5) * 64), lambda h, b: [1, 6, T_H, h["npts"][T_H] + 5]),
    "point_B2": (_flip(lambda h: h["off_pts"][T_B2] + 7 * 128 + 3), lambda h, b: [1, 6, T_B2, 7]),
    "twiddle": (_flip(lambda h: h["off_tw"] + 3 * 32), lambda h, b: [1, 7, 0, 3]),
    "coef_is_r": (lambda buf, h: [(h["off_coef"][0] + 32 * 9, FR_MODULUS.to_bytes(32, "little"))], lambda h, b: [1, 8, 0, 9]),
    "shared_rank_B2": (_unshare_b, lambda h, b: [2, 9, T_B2, _first_b2_entries(h, b)[0]]),
    "delta2": (_flip(lambda h: 552 + 5), lambda h, b: [1, 10, 4, 0]),
}


@pytest.mark.parametrize("case", sorted(VALUES))
def test_value_damage_passes_level0_and_is_named_by_level1(case, tx_key, tmp_path):
    import zkr_hip
    damage, report = VALUES[case]
    blob, h = tx_key["blob"], tx_key["h"]
    want = report(h, blob)
    bad = str(tmp_path / "bad.zkrkey")
    with open(bad, "wb") as f:
        f.write(_apply(blob, damage(blob, h)))
    key = zkr_hip.ProvingKey.load_file(bad)
    try:
        assert key.check(0)["bad"] == 0
        rep = (ctypes.c_uint64 * 4)()
        assert zkr_hip.lib().zkr_key_check(key._h, 1, rep) == -2
        assert list(rep) == want, (list(rep), zkr_hip.lib().zkr_last_error())
        with pytest.raises(zkr_hip.ZkrError) as e:
            key.check(1)
        assert e.value.code == -2 and "key check: %s" % zkr_hip.binding.KEY_SECTIONS[want[1]] in str(e.value)
    finally:
        key.close()


# ---- 5. the Node host
NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(PKG, "napi", "zkr_napi.node")), reason="node or the N-API addon is not available")
def test_node_load_refuses_damage_and_deep_check_passes(tx_key, tmp_path):
    damage, names = STRUCTURAL["col_A"]
    bad = str(tmp_path / "bad.zkrkey")
    with open(bad, "wb") as f:
        f.write(_apply(tx_key["blob"], damage(tx_key["blob"], tx_key["h"])))
    r = subprocess.run([NODE, "-e", """
      const z = require('./index.js');
      (async () => {
        const bn = await z.buildBn128();
        bn.loadKeyFile(process.argv[1]);
        const good = bn.checkKey({deep: true});
        let refused = null;
        const other = await z.buildBn128();
        try { other.loadKeyFile(process.argv[2]); other.terminate(); } catch (e) { refused = e.message; }
        console.log(JSON.stringify({good, refused}));
      })().catch(e => { console.error(e); process.exit(1); });
    """, tx_key["path"], bad], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    import json
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["good"] == {"bad": 0, "section": 0, "part": 0, "first": 0}
    assert res["refused"] is not None and "key check: " + names in res["refused"]
