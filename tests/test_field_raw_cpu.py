"""CPU: every operation of the 8 x 32-bit-limb field (csrc/field.hpp, field_fused.hpp: mul, sqr, add, sub, neg, reduce_once, mul_sum2,
mul_sum4, mul_sub, to_mont, from_mont, inv over Fq and Fr; mul, sqr, mul_sub, inv over Fq2) in its HOST build -- mul_host64, sums
of separate products, the Karatsuba Fq2 product -- on raw limbs at the edges of the operand ranges, against Python integers
(tests/field_cases.py holds the records and what they must give).  Bit for bit, every record, no tolerance: all results are
canonical.  The case lists' own promises (a Montgomery quotient of all ones and of zero, t == p, the ceiling columns, both
outcomes of the last subtraction at least 64 times per reduction) are asserted here too.  The device build does not share this
code: tests/test_gpu_field_raw.py runs the same records through zkr_selftest_fp."""
import ctypes
import os

import pytest

import field_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.environ.get("ZKR_HOSTARITH_LIB") or os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "libzkr_hostarith.so")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SHIM):
        pytest.skip("host arithmetic shim not built (run __graft_entry__.build())")
    return ctypes.CDLL(SHIM)


def fp_raw_host(L, field, num, data, out_words):
    """zkt_fp_raw on n x 256 bytes of records: the result bytes."""
    n = len(data) // 256
    out = (ctypes.c_uint32 * max(1, out_words * n))()
    L.zkt_fp_raw.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    L.zkt_fp_raw.restype = None
    L.zkt_fp_raw(field, num, data, n, out)
    return bytes(out)[:4 * out_words * n]


def host_results(L, cs):
    return fp_raw_host(L, cs.field, cs.num, cs.data, cs.out_words)


def test_the_op_table_is_the_one_the_header_reads():
    """One list of operations (csrc/field_raw_ops.def): numbered 0 .. 15 in the order the issue of this hook fixed."""
    assert fc.OP_NAMES == ("mul", "sqr", "add", "sub", "neg", "reduce_once", "mul_sum2", "mul_sum4", "mul_sub", "to_mont", "from_mont", "inv",
                           "fq2_mul", "fq2_sqr", "fq2_mul_sub", "fq2_inv")
    assert [fc.OPS[n][1] for n in fc.OP_NAMES] == [2, 1, 2, 2, 1, 1, 4, 8, 4, 1, 1, 1, 4, 2, 8, 2]
    assert [fc.OPS[n][2] for n in fc.OP_NAMES] == [8] * 12 + [16] * 4
    assert len(fc.PARAMS) == 28


@pytest.mark.parametrize("field,name", fc.PARAMS, ids=fc.IDS)
def test_host_build_on_raw_limbs_equals_the_integers(L, field, name):
    cs = fc.cases(field, name)
    assert fc.check_against(cs, host_results(L, cs), cs.want, cs.kinds, cs.ops, "host build") == len(cs.ops)
    for n in fc.BATCH_SIZES:
        data, kinds, ops, want = cs.batch(n)
        assert fc.check_against(cs, fp_raw_host(L, field, cs.num, data, cs.out_words), want, kinds, ops, "host build, batch of %d" % n) == n


@pytest.mark.parametrize("field,name", [pn for pn in fc.PARAMS if pn[1] in fc.PRODUCT_OPS + fc.INV_OPS], ids=[i for i, pn in zip(fc.IDS, fc.PARAMS) if pn[1] in fc.PRODUCT_OPS + fc.INV_OPS])
def test_records_reach_both_outcomes_of_the_last_subtraction(field, name):
    """Conditions on the INPUTS, from the model of the device's reduction in field_cases.py: for every reduction of the op, t >= p in
    at least 64 records and t < p in at least 64 (random operands alone give t >= p 4.8 % of the time for mul)."""
    cs = fc.cases(field, name)
    assert cs.reach and len(cs.reach) == (1 if name in fc.INV_OPS else len(fc.device_sums(cs.p, name, [1] * 8)))
    for slot, (n_ge, n_lt) in enumerate(cs.reach):
        assert n_ge >= fc.MIN_REACH and n_lt >= fc.MIN_REACH, (name, slot, n_ge, n_lt)


def test_records_hold_the_extreme_quotients_and_every_pattern():
    for field, p in enumerate(fc.MODULI):
        for name in ("mul", "mul_sum2", "mul_sum4"):
            cs = fc.cases(field, name)
            pairs = cs.n_in // 2
            ms = [fc.redc(p, sum(o[2 * k] * o[2 * k + 1] for k in range(pairs))) for o in cs.ops]
            assert sum(1 for t, m in ms if m == fc.W - 1) >= 16 and sum(1 for t, m in ms if m == 0 and t == 1) >= 14
            assert sum(1 for t, m in ms if t == p) >= 12
            top = fc.top_value(p)
            assert top < p and top & ((1 << 224) - 1) == (1 << 224) - 1 and 4 * top * top < p * fc.W
            assert tuple([top] * cs.n_in) in [o[:cs.n_in] for o in cs.ops] and tuple([p] * cs.n_in) in [o[:cs.n_in] for o in cs.ops]
        for name in fc.OP_NAMES if field == 0 else fc.OP_NAMES[:12]:
            cs = fc.cases(field, name)
            for k in range(cs.n_in):                       # every pattern in every operand position
                assert set(cs.pats) <= set(o[k] for o in cs.ops), (name, k)
            assert all(0 <= v <= cs.hi for o in cs.ops for v in o[:cs.n_in])
    assert fc.bound(fc.Q, "reduce_once") == fc.W - 1 and fc.W - 1 in fc.patterns(fc.Q, fc.W - 1)


def test_device_hook_refuses_bad_arguments():
    """zkr_selftest_fp refuses null pointers and an op or field out of range with ZKR_ERR_ARG (-5) before any HIP work, as the two
    hooks beside it do: no device needed."""
    import zkr_hip
    Lh = zkr_hip.lib()
    rec, out = (ctypes.c_uint32 * 64)(), (ctypes.c_uint32 * 16)()
    f = Lh.zkr_selftest_fp
    assert f(0, 0, 0, None, 1, out) == -5 and f(0, 0, 0, rec, 1, None) == -5
    assert b"bad argument" in Lh.zkr_last_error()
    assert f(0, 0, -1, rec, 1, out) == -5 and f(0, 0, 16, rec, 1, out) == -5
    assert f(0, 2, 0, rec, 1, out) == -5 and f(0, -1, 0, rec, 1, out) == -5
    for op in (12, 13, 14, 15):                            # Fq2 stands over Fq only
        assert f(0, 1, op, rec, 1, out) == -5
    assert f(0, 0, 0, rec, (1 << 24) + 1, out) == -5 and b"too many records" in Lh.zkr_last_error()
    with pytest.raises(ValueError):
        zkr_hip.selftest_fp(0, "mul", bytes(255))
    with pytest.raises(KeyError):
        zkr_hip.selftest_fp(0, "cube", bytes(256))
