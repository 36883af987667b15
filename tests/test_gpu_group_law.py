"""GPU: the group law of the hot path as the DEVICE compiles it (csrc/curve29.hpp with every product one opaque asm statement, a
scheduling barrier between products and the special cases as per-lane branches), on the raw-limb records of tests/curve29_cases.py
through zkr_selftest_curve29: coordinates at the bounds their types declare, curve points in non-canonical clothes, the forced full
zero test over Fq2; every branch in every wavefront, one wavefront all general, one all doubling, a ragged tail.  Compared with
integer arithmetic (the same four assertions as the host build gets in tests/test_group_law_bounds_cpu.py) and with the host
build of the same header limb for limb -- the contract the product forms already have, one layer up."""
import ctypes
import os

import pytest

import curve29_cases as cc

pytestmark = pytest.mark.gpu

PARAMS = [(g2, op) for g2 in (0, 1) for op in cc.OPS]
IDS = ["%s-%s" % ("G2" if g2 else "G1", cc.OP_NAMES[op].replace("/", "+")) for g2, op in PARAMS]
_device_results = {}


def _device(g2, op):
    """One launch per (group, op), shared by the two tests."""
    if (g2, op) not in _device_results:
        import zkr_hip
        _device_results[(g2, op)] = zkr_hip.selftest_curve29(g2, op, cc.cases(g2, op).words())
    return _device_results[(g2, op)]


@pytest.mark.parametrize("g2,op", PARAMS, ids=IDS)
def test_device_group_law_at_its_declared_bounds_equals_the_integers(g2, op):
    out, inf = _device(g2, op)
    assert cc.check_results(cc.cases(g2, op), out, inf, "device") == cc.N_RECORDS


@pytest.mark.parametrize("g2,op", PARAMS, ids=IDS)
def test_device_group_law_equals_the_host_build_limb_for_limb(g2, op):
    from test_group_law_bounds_cpu import SHIM, curve_raw_host
    assert os.path.exists(SHIM), "host arithmetic shim not built (run __graft_entry__.build())"
    cs = cc.cases(g2, op)
    out, inf = _device(g2, op)
    h_out, h_inf = curve_raw_host(ctypes.CDLL(SHIM), cs)
    assert inf == h_inf, "infinity flags differ at records %s" % [i for i in range(cc.N_RECORDS) if inf[i] != h_inf[i]][:8]
    if out != h_out:
        ow = cc.words_per(g2, op)[1]
        bad = [i for i in range(cc.N_RECORDS) if out[i * ow:(i + 1) * ow] != h_out[i * ow:(i + 1) * ow]]
        raise AssertionError("%s %s: %d records differ limb for limb, first %s (%s, %s)" % (
            "G2" if g2 else "G1", cc.OP_NAMES[op], len(bad), bad[:8], cs.recs[bad[0]].family, cs.branch[bad[0]]))
