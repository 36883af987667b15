"""GPU: the 8 x 32-bit-limb field as the DEVICE compiles it -- mul by product scanning in a 96-bit column accumulator (the mac96*
asm statements of csrc/field.hpp, the modulus words as template constants), mul_sum2 / mul_sum4 as one fused scan
(csrc/field_fused.hpp), the schoolbook Fq2 product and both mul_sub through them with negated operands: code the host build
does not share -- on the raw-limb records of tests/field_cases.py through zkr_selftest_fp.  Every (field, op): the device's words
equal the Python integers and equal the host build of the same function (zkt_fp_raw), bit for bit, over the whole list and over
batches of 1, 64 and 65 records (a lone lane, a full wavefront, one lane into the next).  A failure names the first differing
record with its kind and operands."""
import ctypes
import os

import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

_device_results = {}


def _device(field, name):
    """One launch per (field, op) over the whole list, shared by the two tests."""
    if (field, name) not in _device_results:
        import zkr_hip
        _device_results[(field, name)] = zkr_hip.selftest_fp(field, name, fc.cases(field, name).data)
    return _device_results[(field, name)]


@pytest.mark.parametrize("field,name", fc.PARAMS, ids=fc.IDS)
def test_device_field_on_raw_limbs_equals_the_integers(field, name):
    import zkr_hip
    cs = fc.cases(field, name)
    assert fc.check_against(cs, _device(field, name), cs.want, cs.kinds, cs.ops, "device") == len(cs.ops)
    for n in fc.BATCH_SIZES:
        data, kinds, ops, want = cs.batch(n)
        assert fc.check_against(cs, zkr_hip.selftest_fp(field, cs.num, data), want, kinds, ops, "device, batch of %d" % n) == n
    assert zkr_hip.selftest_fp(field, name, b"") == b""


@pytest.mark.parametrize("field,name", fc.PARAMS, ids=fc.IDS)
def test_device_field_equals_the_host_build_bit_for_bit(field, name):
    from test_field_raw_cpu import SHIM, host_results
    assert os.path.exists(SHIM), "host arithmetic shim not built (run __graft_entry__.build())"
    cs = fc.cases(field, name)
    host = fc.ints(host_results(ctypes.CDLL(SHIM), cs), cs.n_out)
    assert fc.check_against(cs, _device(field, name), host, cs.kinds, cs.ops, "device", "the host build") == len(cs.ops)
