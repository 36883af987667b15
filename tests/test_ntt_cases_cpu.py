"""CPU: the reference of tests/ntt_cases.py -- what tests/test_gpu_ntt_modes.py holds the device's NTT launches to -- against a
direct O(n^2) evaluation of each mode's definition, against the pass model of tests/test_ntt_plan.py (the kernel's index math) and
against itself: the cross stages composed with the blocks' own transforms are the whole transform, and the coset factors of a block
(shift / add) are the whole transform's."""
import random

import numpy as np
import pytest

import groth16 as g
import ntt_cases as nc
from bn254 import R
from test_ntt_plan import bitrev, make_tw, run_ntt

DIRECTIONS = [(True, False), (True, True), (False, False), (False, True)]   # (dif, inverse)


def direct(x, L, dif, inverse):
    """The definition, term by term: X = the input in natural order (a DIT transform takes it bit-reversed), S[i] = sum_k X[k] w^(+-i k)
    without the 1/n of an inverse, stored at br(i) by a DIF transform and at i by a DIT one."""
    n = 1 << L
    w = g.root_of_unity(n)
    pw = [pow(w, e, R) for e in range(n)]
    X = x if dif else [x[bitrev(i, L)] for i in range(n)]
    out = [None] * n
    for i in range(n):
        s = sum(X[k] * pw[(-i * k if inverse else i * k) % n] for k in range(n)) % R
        out[bitrev(i, L) if dif else i] = s
    return out


@pytest.mark.parametrize("L", range(3, 9))
def test_every_mode_equals_its_definition_and_the_pass_model(L):
    rnd = random.Random(0x4E77 + L)
    n = 1 << L
    a = [rnd.randrange(R) for _ in range(n)]
    b = [rnd.randrange(R) for _ in range(n)]
    a[0] = R - 1
    tw, twl = make_tw(n), make_tw(8)
    gen = g.root_of_unity(2 * n)
    for dif, inverse in DIRECTIONS:
        desc = dict(logn=L, dif=dif, inverse=inverse)
        want = direct(a, L, dif, inverse)
        assert nc.plain_expected(desc, a) == want, desc
        model = list(a)
        run_ntt(model, L, dif, inverse, tw, L, twl, 3)       # the kernel's index math, scaled down (tile 2^4, local table 2^3)
        assert model == want, desc
        assert nc.transform_bytes(nc.pack(a), L, dif, inverse) == nc.pack(want), desc
        # PRE_COSET on the whole transform, PRE_MUL
        cos = [v * pow(gen, bitrev(gi, L), R) % R for gi, v in enumerate(a)]
        assert nc.plain_expected(dict(desc, pre=nc.PRE_COSET, tlog=L), a) == direct(cos, L, dif, inverse), desc
        prod = [x * y * pow(1 << 256, R - 2, R) % R for x, y in zip(a, b)]
        assert nc.plain_expected(dict(desc, pre=nc.PRE_MUL), a, b) == direct(prod, L, dif, inverse), desc
    # an inverse transform is n times the oracle's
    assert [v * n % R for v in g.ntt(a, invert=True)] == [nc.plain_expected(dict(logn=L, dif=True, inverse=True), a)[bitrev(i, L)] for i in range(n)]
    # vectors end to end are independent transforms
    two = nc.plain_expected(dict(logn=L, dif=True, inverse=True, nbat=2, pre=nc.PRE_MUL), a + b, b + a)
    assert two[:n] == two[n:] == nc.plain_expected(dict(logn=L, dif=True, inverse=True, pre=nc.PRE_MUL), a, b)


def test_both_oracles_give_the_same_transform_across_the_threshold():
    rnd = random.Random(99)
    for L in (nc.ORACLE_SMALL_LOG, nc.ORACLE_SMALL_LOG + 1):
        a = [rnd.randrange(R) for _ in range(1 << L)]
        assert nc.oracle_ntt(a) == g.ntt(a) == nc.unpack(nc.coracle.ntt(nc.pack(a)))
    assert nc.bitrev_perm(5).tolist() == [bitrev(i, 5) for i in range(32)] and nc.bitrev_perm(1).tolist() == [0, 1]


@pytest.mark.parametrize("L,klog", [(3, 1), (5, 2), (7, 3), (8, 1), (8, 2), (8, 3)])
def test_cross_stages_and_the_blocks_own_transforms_make_the_whole_transform(L, klog):
    """The identity of tests/test_shard_eval_plan.py with this module's functions: an inverse DIF transform is its top klog stages
    across the row blocks, then an inverse DIF transform of every block; a forward DIT transform with the coset factors is a forward
    DIT transform of every block with the block's factors (shift = klog, add = the block's index bit-reversed), then the top stages."""
    rnd = random.Random(1000 * L + klog)
    n, rows, Lb = 1 << L, 1 << klog, L - klog
    Bk = n >> klog
    a = [rnd.randrange(R) for _ in range(n)]
    b = [rnd.randrange(R) for _ in range(n)]
    for pre, x in ((nc.PRE_NONE, a), (nc.PRE_MUL, nc.pre_apply(nc.PRE_MUL, a, b, L))):
        top = nc.cross_expected(x, L, klog, True, True)
        split = []
        for r in range(rows):
            split += nc.plain_expected(dict(logn=Lb, dif=True, inverse=True), top[r * Bk:(r + 1) * Bk])
        assert split == nc.plain_expected(dict(logn=L, dif=True, inverse=True, pre=pre), a, b if pre else None)
    low = []
    for r in range(rows):
        low += nc.plain_expected(dict(logn=Lb, dif=False, inverse=False, pre=nc.PRE_COSET, tlog=L, coset_shift=klog, coset_add=bitrev(r, klog)), a[r * Bk:(r + 1) * Bk])
    assert nc.cross_expected(low, L, klog, False, False) == nc.plain_expected(dict(logn=L, dif=False, inverse=False, pre=nc.PRE_COSET, tlog=L), a)
    # the forward DIF and inverse DIT cross passes, which no proof runs, the same way
    top = nc.cross_expected(a, L, klog, True, False)
    assert sum((nc.plain_expected(dict(logn=Lb, dif=True, inverse=False), top[r * Bk:(r + 1) * Bk]) for r in range(rows)), []) == \
        nc.plain_expected(dict(logn=L, dif=True, inverse=False), a)
    low = sum((nc.plain_expected(dict(logn=Lb, dif=False, inverse=True), a[r * Bk:(r + 1) * Bk]) for r in range(rows)), [])
    assert nc.cross_expected(low, L, klog, False, True) == nc.plain_expected(dict(logn=L, dif=False, inverse=True), a)


@pytest.mark.parametrize("L,klog", [(4, 1), (6, 2), (8, 3), (8, 1)])
def test_block_coset_factors_are_the_whole_transforms(L, klog):
    """Position gi of block r is position (r << (L - klog)) + gi of the whole vector: the exponent of g that PRE_COSET gives it
    with (shift, add) = (klog, br(r)) and tlog = L is the whole transform's br(position) -- and with a table of a LARGER transform
    (tlog > L) both scale by the same power of two."""
    Lb = L - klog
    for r in range(1 << klog):
        for gi in range(1 << Lb):
            assert nc.coset_exponent(gi, Lb, L, klog, bitrev(r, klog)) == nc.coset_exponent((r << Lb) + gi, L, L, 0, 0) == bitrev((r << Lb) + gi, L)
            assert nc.coset_exponent(gi, Lb, L + 2, klog, bitrev(r, klog)) == bitrev((r << Lb) + gi, L) << 2
    rnd = random.Random(L)
    a = [rnd.randrange(R) for _ in range(1 << L)]
    whole = nc.pre_apply(nc.PRE_COSET, a, None, L, L)
    gen = g.root_of_unity(2 << L)
    assert whole == [v * pow(gen, bitrev(p, L), R) % R for p, v in enumerate(a)]
    blocks = []
    for r in range(1 << klog):
        blocks += nc.pre_apply(nc.PRE_COSET, a[r << Lb:(r + 1) << Lb], None, Lb, L, klog, bitrev(r, klog))
    assert blocks == whole


def test_cross_vectors_and_check_cross_accept_the_model_and_refuse_a_wrong_column():
    """The comparison itself: the model's own output passes in every layout the hook has; one wrong word, a non-canonical word where
    canonical ones are due, a word of 3 r or more, and a touched column outside the shard's all fail."""
    L, klog = 7, 2
    rows, Bk = 1 << klog, 1 << (L - klog)
    rnd = random.Random(5)
    x = [rnd.randrange(R) for _ in range(1 << L)]
    want = nc.cross_expected(x, L, klog, True, True)
    for lo, cn, in_sub, out_sub, canon in ((0, 8, 0, 0, 0), (24, 8, 0, 24, 1), (24, 8, 24, 0, 0), (8, 16, 0, 0, 1)):
        desc = dict(logn=L, klog=klog, cross=1, dif=1, inverse=1, col_lo=lo, col_n=cn, in_sub=in_sub, out_sub=out_sub, canon=canon)
        width = cn if out_sub else Bk
        out = [None] * (rows * width)
        fill = int.from_bytes(bytes([nc.FILL]) * 32, "little")
        for r in range(rows):
            for c in range(width):
                col = c + out_sub
                out[r * width + c] = want[r * Bk + col] + (0 if canon else R) if lo <= col < lo + cn else fill
        got = dict(in0=nc.cross_vectors(desc, x), out=nc.pack(out))
        assert len(got["in0"]) == 32 * rows * (cn if in_sub else Bk)
        nc.check_cross(desc, got, want, x)
        at = (rows - 1) * width + lo - out_sub
        for wrong in (out[at] + 1, out[at] + (R if canon else 2 * R)):
            bad = list(out)
            bad[at] = wrong
            with pytest.raises(AssertionError):
                nc.check_cross(desc, dict(got, out=nc.pack(bad)), want, x)
        if not out_sub:
            bad = list(out)
            bad[(lo + cn) % Bk if lo + cn < Bk else lo - 1] ^= 1
            with pytest.raises(AssertionError):
                nc.check_cross(desc, dict(got, out=nc.pack(bad)), want, x)
        with pytest.raises(AssertionError):
            nc.check_cross(desc, dict(got, in0=got["in0"][:-1] + b"\x01"), want, x)


def test_check_plain_compares_the_wanted_range_only_and_the_inputs():
    L = 6
    rnd = random.Random(6)
    a = [rnd.randrange(R) for _ in range(1 << L)]
    desc = dict(logn=L, dif=1, inverse=1, want_lo=16, want_n=8)
    want = nc.plain_expected(desc, a)
    junk = [7] * 16 + want[16:24] + [9] * 40
    nc.check_plain(desc, dict(in0=nc.pack(a), out=nc.pack(junk)), a)
    for at in (16, 23):
        bad = list(junk)
        bad[at] += 1
        with pytest.raises(AssertionError):
            nc.check_plain(desc, dict(in0=nc.pack(a), out=nc.pack(bad)), a)
    with pytest.raises(AssertionError):
        nc.check_plain(desc, dict(in0=nc.pack(a[1:] + a[:1]), out=nc.pack(junk)), a)
    with pytest.raises(AssertionError):
        nc.check_plain(dict(desc, want_n=0, want_lo=0), dict(in0=nc.pack(a), out=nc.pack(junk)), a)
    nc.check_plain(dict(desc, in_place=1), dict(in0=nc.pack(junk)), a)


def test_the_hook_refuses_bad_descriptors_before_any_device_work():
    """zkr_selftest_ntt checks every field of its descriptor on the host, before it looks for a device: each bad value is
    ZKR_ERR_ARG (-5) with a message on a machine without a GPU too, and a ragged vector never reaches the C side."""
    import zkr_hip
    v = bytes(32 * 256)
    plain, cross = dict(logn=8, dif=1, inverse=1), dict(logn=8, dif=1, inverse=1, cross=1, klog=2, col_lo=16, col_n=16)
    bad = [dict(plain, logn=0), dict(plain, logn=23), dict(plain, dif=2), dict(plain, inverse=2), dict(plain, pre=3), dict(plain, pair=2),
           dict(plain, in_place=2), dict(plain, nbat=0), dict(plain, nbat=1 << 17), dict(plain, tlog=7), dict(plain, tlog=25), dict(plain, reserved=1),
           dict(plain, pre=1, coset_shift=1, tlog=8), dict(plain, pre=1, coset_shift=1, coset_add=2, tlog=9), dict(plain, coset_shift=1, tlog=9),
           dict(plain, coset_add=1), dict(plain, klog=1), dict(plain, col_n=4), dict(plain, canon=1), dict(plain, in_sub=1), dict(plain, out_sub=1),
           dict(cross, klog=0), dict(cross, klog=4), dict(cross, logn=2, klog=2, col_lo=0, col_n=1), dict(cross, nbat=2), dict(cross, pair=1),
           dict(cross, want_n=1), dict(cross, pre=1), dict(cross, col_n=0), dict(cross, col_lo=56, col_n=16), dict(cross, col_lo=8, col_n=16),
           dict(cross, col_n=24), dict(cross, in_sub=8), dict(cross, out_sub=32), dict(cross, in_place=1, out_sub=16), dict(cross, canon=2)]
    for desc in bad:
        n_in, n_out = zkr_hip.ntt_selftest_words(desc) or (1, 1)
        i, o = bytes(32 * n_in), bytes(32 * n_out)
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.selftest_ntt(desc, i, i, o, i, i, o)
        assert e.value.code == -5 and "zkr_selftest_ntt" in str(e.value), desc
    for missing in (dict(in0=None), dict(out=None), dict(plain_extra=dict(pre=2), in1=None), dict(plain_extra=dict(pair=1), in0_b=None),
                    dict(plain_extra=dict(pair=1), out_b=None), dict(plain_extra=dict(pair=1, pre=2), in1_b=None)):
        desc = dict(plain, **missing.pop("plain_extra", {}))
        vecs = dict(dict(in0=v, in1=v, out=v, in0_b=v, in1_b=v, out_b=v), **missing)
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.selftest_ntt(desc, **vecs)
        assert e.value.code == -5 and "null" in str(e.value), missing
    assert zkr_hip.lib().zkr_selftest_ntt(0, None, v, v, v, v, v, v) == -5
    for desc, vecs in ((plain, dict(in0=v[:-32], out=v)), (plain, dict(in0=v, out=v + v)), (cross, dict(in0=v, out=v[:32])),
                       (dict(cross, in_sub=16), dict(in0=v, out=v)), (dict(plain, nbat=2), dict(in0=v, out=v))):
        with pytest.raises(ValueError):
            zkr_hip.selftest_ntt(desc, **vecs)
    with pytest.raises(ValueError):
        zkr_hip.selftest_ntt(dict(plain, colour=1), v, out=v)
    if zkr_hip.device_count() == 0:     # a good descriptor gets as far as the device
        for desc in (plain, cross, dict(cross, in_sub=16, out_sub=0, pre=2)):
            with pytest.raises(zkr_hip.ZkrError) as e:
                zkr_hip.selftest_ntt(desc, v if not desc.get("in_sub") else v[:32 * 64], v if not desc.get("in_sub") else v[:32 * 64], v)
            assert e.value.code == -1, desc


def test_cross_wlog_is_the_drivers():
    assert [nc.cross_wlog(k, c) for k, c in ((1, 1), (1, 2), (2, 16), (2, 1024), (3, 2048), (3, 256), (1, 4096))] == [0, 1, 4, 9, 8, 8, 10]
    assert isinstance(nc.bitrev_perm(3), np.ndarray)
