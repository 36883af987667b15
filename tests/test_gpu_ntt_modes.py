"""GPU: the NTT pass kernel (csrc/kernels_ntt.hpp ntt_pass_kernel) in every mode the prover's two drivers launch it in, each mode
ALONE: one run_ntt or one run_ntt_cross of csrc/zkr_prove.hip through zkr_selftest_ntt -- the code objects the proofs launch -- on
vectors of this file, the raw result compared with the integer reference of tests/ntt_cases.py (checked without a GPU by
tests/test_ntt_cases_cpu.py).  Exact equality everywhere, no tolerance: the last pass of a transform stores canonical residues; a
cross pass that does not is compared mod r after every stored word is seen to be below 3 r.  Every device vector lies between
guard regions which the hook reads back after the run: a launch that writes outside its vector fails the call."""
import functools
import random

import numpy as np
import pytest

import ntt_cases as nc
from bn254 import R

pytestmark = pytest.mark.gpu

DIRECTIONS = [(1, 0), (1, 1), (0, 0), (0, 1)]      # (dif, inverse); the prover runs DIF inverse and DIT forward
DIR_IDS = ["dif-fwd", "dif-inv", "dit-fwd", "dit-inv"]
ONES29 = ((1 << 253) - 1) % R                      # every 29-bit limb all ones


@functools.lru_cache(maxsize=None)
def vec(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(R) for _ in range(n)]


def fill(n):
    return bytes([nc.FILL]) * (32 * n)


def run_plain(desc, in0, in1=None, in0_b=None, in1_b=None):
    import zkr_hip
    n = desc.get("nbat", 1) << desc["logn"]
    assert len(in0) == n
    out = None if desc.get("in_place", 0) else fill(n)
    pair = desc.get("pair", 0)
    got = zkr_hip.selftest_ntt(desc, nc.pack(in0), None if in1 is None else nc.pack(in1), out, nc.pack(in0_b) if pair else None,
                               nc.pack(in1_b) if pair and in1_b is not None else None, out if pair else None)
    nc.check_plain(desc, got, in0, in1, in0_b, in1_b)


# ------------------------------------------------------------------------------------------------ whole transforms, PRE_NONE
@pytest.mark.parametrize("dif,inverse", DIRECTIONS, ids=DIR_IDS)
@pytest.mark.parametrize("L", [1, 2, 3, 4, 7, 10, 11, 12, 13, 15, 16])
def test_every_direction_alone(L, dif, inverse):
    """One contiguous pass with odd and even stage counts, the 256-thread small tiles (L <= 10), strided passes of 1, 2, 4 and 5 stages
    in front of (DIF) or behind (DIT) the full tile.  The DIT inverse kernels are launched by nothing else."""
    v = list(vec(L, 1 << L))
    v[0] = R - 1
    run_plain(dict(logn=L, dif=dif, inverse=inverse), v)


def structured(L):
    n = 1 << L
    rnd = random.Random(2000 + L)
    return {"all r - 1": [R - 1] * n,
            "0 or r - 1": [(R - 1) if rnd.random() < 0.5 else 0 for _ in range(n)],
            "one entry at 0": [R - 1] + [0] * (n - 1),
            "one entry at n - 1": [0] * (n - 1) + [R - 1],
            "alternating r - 1, 1": [R - 1, 1] * (n // 2),
            "limbs all ones": [ONES29] * n}


@pytest.mark.parametrize("dif,inverse", DIRECTIONS, ids=DIR_IDS)
@pytest.mark.parametrize("L", [11, 13, 15])
def test_structured_inputs_in_every_direction(L, dif, inverse):
    """The lazily reduced butterflies at the top of their bounds (kernels_ntt.hpp NTT_H_*), DIT included: sums grow by up to 4 half
    moduli per stage of a DIT pass and are reduced once, when the pass stores; a DIF pair of stages quadruples one output.  All r - 1
    and 0 / r - 1 drive the sums; a single entry leaves every butterfly one zero operand; r - 1, 1 alternating puts DIT sums at
    their maximum and differences at zero in alternate stages; (2^253 - 1) mod r has every limb full."""
    for name, v in structured(L).items():
        try:
            run_plain(dict(logn=L, dif=dif, inverse=inverse), v)
        except AssertionError as e:
            raise AssertionError("input %r: %s" % (name, e))


@functools.lru_cache(maxsize=None)
def natural_2_21():
    """2^21 words below 2^253 < r as bytes, natural order"""
    rows = np.random.default_rng(21).integers(0, 256, size=(1 << 21, 32), dtype=np.uint8)
    rows[:, 31] &= 0x1F
    rows[0] = np.frombuffer(nc.pack([R - 1]), dtype=np.uint8)
    return rows


@pytest.mark.parametrize("dif,inverse", [(1, 1), (0, 0)], ids=["dif-inv", "dit-fwd"])
def test_2_21_in_the_directions_the_prover_runs(dif, inverse):
    """The smallest transform on 256-thread workgroups with full 2048-element tiles (NTT_LARGE_LOG) and the first with two strided
    passes (5 + 5 stages), which no other test runs at all.  Both directions transform the same natural-order vector, so the C
    oracle runs once."""
    import zkr_hip
    L = 21
    rows = natural_2_21()
    data = (rows if dif else rows[nc.bitrev_perm(L)]).tobytes()
    got = zkr_hip.selftest_ntt(dict(logn=L, dif=dif, inverse=inverse), data, out=fill(1 << L))
    assert got["in0"] == data
    want = nc.transform_bytes(data, L, bool(dif), bool(inverse))
    if got["out"] != want:
        a, b = np.frombuffer(got["out"], dtype=np.uint8).reshape(-1, 32), np.frombuffer(want, dtype=np.uint8).reshape(-1, 32)
        wrong = np.nonzero((a != b).any(axis=1))[0]
        raise AssertionError("%d of 2^21 words differ, first at position %d" % (len(wrong), wrong[0]))


# ------------------------------------------------------------------------------------------------ the first pass's extra work
@pytest.mark.parametrize("L", [4, 11, 13])
def test_coset_factors_and_products_alone(L):
    """PRE_COSET as calcH runs it (forward DIT on the whole domain, table of the transform's own size) and PRE_MUL (inverse DIF): the
    product of two standard-form words keeps its factor 2^-256 here, where calcH folds it into two constants."""
    n = 1 << L
    run_plain(dict(logn=L, dif=0, inverse=0, pre=nc.PRE_COSET, tlog=L), vec(10 + L, n))
    run_plain(dict(logn=L, dif=1, inverse=1, pre=nc.PRE_MUL), vec(20 + L, n), vec(30 + L, n))


@pytest.mark.parametrize("shift,add", [(1, 0), (1, 1), (3, 5)])
@pytest.mark.parametrize("L", [8, 12])
def test_coset_factors_of_a_block_of_a_larger_transform(L, shift, add):
    """pre_shift / pre_add with a table 2^shift times the transform: block `add` (bit-reversed) of a split calcH."""
    run_plain(dict(logn=L, dif=0, inverse=0, pre=nc.PRE_COSET, tlog=L + shift, coset_shift=shift, coset_add=add), vec(40 + L + shift, 1 << L))


@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("nbat", [1, 3])
@pytest.mark.parametrize("L", [5, 12])
def test_fused_batches_and_paired_launches(L, nbat, pair, in_place):
    """blockIdx.y (vectors end to end) and gridDim.z = 2 (the *_b pointers) for the three calls of calc_h_device, in place and out of
    place.  Every vector is different, so a swapped pointer or a wrong batch stride shows; out of place the inputs come back
    unchanged (check_plain)."""
    n = nbat << L
    a, b, c, d = (vec(100 * L + 10 * nbat + k, n) for k in range(4))
    common = dict(logn=L, nbat=nbat, pair=pair, in_place=in_place)
    run_plain(dict(common, dif=1, inverse=1), a, None, c if pair else None, None)
    run_plain(dict(common, dif=0, inverse=0, pre=nc.PRE_COSET, tlog=L), a, None, c if pair else None, None)
    run_plain(dict(common, dif=1, inverse=1, pre=nc.PRE_MUL), a, b, c if pair else None, d if pair else None)


# ------------------------------------------------------------------------------------------------ output ranges
def ranges(L):
    n = 1 << L
    return [(0, 1), (n - 1, 1), (2047, 2), (2048, 2048), (3000, 5000), (n // 2 - 1, 2), (0, n)]


@pytest.mark.parametrize("which", range(7))
@pytest.mark.parametrize("L", [13, 16])
def test_output_ranges_of_an_inverse_dif_transform(L, which):
    """want_lo / want_n -> blk_off: the passes below the top one run on the aligned blocks that cover the range, and the range must
    come out whole -- out of place and alone, and as calc_h_device asks for it: products, a pair, in place."""
    lo, cnt = ranges(L)[which]
    n = 1 << L
    run_plain(dict(logn=L, dif=1, inverse=1, want_lo=lo, want_n=cnt), vec(50 + L, n))
    run_plain(dict(logn=L, dif=1, inverse=1, pre=nc.PRE_MUL, pair=1, in_place=1, want_lo=lo, want_n=cnt), vec(51 + L, n), vec(52 + L, n), vec(53 + L, n), vec(54 + L, n))


def test_refused_ranges():
    """run_ntt's own refusals, through the hook: a range of a DIT transform, a range that leaves the transform."""
    import zkr_hip
    v = nc.pack(vec(60, 1 << 12))
    for desc in (dict(logn=12, dif=0, inverse=0, want_lo=0, want_n=16), dict(logn=12, dif=0, inverse=1, want_lo=5, want_n=1),
                 dict(logn=12, dif=1, inverse=1, want_lo=4095, want_n=2), dict(logn=12, dif=1, inverse=1, want_lo=4096, want_n=1),
                 dict(logn=12, dif=1, inverse=1, want_lo=0xFFFFFFFF, want_n=2)):
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.selftest_ntt(desc, v, out=fill(1 << 12))
        assert e.value.code == -5 and "range" in str(e.value), desc


# ------------------------------------------------------------------------------------------------ cross passes
CROSS_SIZES = sorted({(k, L) for k in (1, 2, 3) for L in (2 * k + 1, 8, 12)} | {(2, 14), (3, 17)})


@functools.lru_cache(maxsize=None)
def cross_reference(klog, L):
    """the inputs of one size and the model's stages [L - klog, L) on them, once for every part and layout"""
    n = 1 << L
    x, y = vec(7000 + 10 * L + klog, n), vec(8000 + 10 * L + klog, n)
    xy = nc.pre_apply(nc.PRE_MUL, x, y, L)
    return dict(x=x, y=y, none={(dif, inv): nc.cross_expected(x, L, klog, bool(dif), bool(inv)) for dif, inv in DIRECTIONS},
                mul=nc.cross_expected(xy, L, klog, True, True))


def run_cross(desc, want, x, y=None):
    import zkr_hip
    rows, Bk = 1 << desc["klog"], 1 << (desc["logn"] - desc["klog"])
    out = None if desc.get("in_place", 0) else fill(rows * (desc["col_n"] if desc.get("out_sub", 0) else Bk))
    got = zkr_hip.selftest_ntt(desc, nc.cross_vectors(desc, x), None if y is None else nc.cross_vectors(desc, y), out)
    nc.check_cross(desc, got, want, x, y)


@pytest.mark.parametrize("last_part", [0, 1], ids=["first-part", "last-part"])
@pytest.mark.parametrize("klog,L", CROSS_SIZES)
def test_cross_passes_alone(klog, L, last_part):
    """run_ntt_cross with each of the 2^klog row blocks in a device allocation of its own, for the columns of the first and the last
    shard of a split calcH (col_n = 2^(L - 2 klog)): the narrow col_n of the small sizes lower the tile width, (2, 14) and (3, 17)
    reach the 2^11 cap with several tiles per launch.  The five calls of calc_h_split with its (in_sub, out_sub) -- whole
    blocks both ways, local columns out, local columns in -- then the evaluation form's in-place pass and the two directions no
    proof runs."""
    ref = cross_reference(klog, L)
    x, y = ref["x"], ref["y"]
    cn = 1 << (L - 2 * klog)
    lo = ((1 << klog) - 1) * cn if last_part else 0
    base = dict(logn=L, klog=klog, cross=1, col_lo=lo, col_n=cn)
    inv_dif, fwd_dit = dict(base, dif=1, inverse=1), dict(base, dif=0, inverse=0, canon=1)
    run_cross(inv_dif, ref["none"][1, 1], x)                                            # phase 2: iNTT(a), iNTT(b)
    run_cross(dict(inv_dif, pre=nc.PRE_MUL), ref["mul"], x, y)                          # phase 2: iNTT(a.b)
    run_cross(fwd_dit, ref["none"][0, 0], x)                                            # phase 4, canonical
    run_cross(dict(fwd_dit, out_sub=lo), ref["none"][0, 0], x)                          # phase 4 into local columns
    run_cross(dict(inv_dif, pre=nc.PRE_MUL, in_sub=lo), ref["mul"], x, y)               # phase 4: the product of local columns
    run_cross(dict(fwd_dit, in_place=1), ref["none"][0, 0], x)                          # evaluation form: phase 4 in place
    run_cross(dict(base, dif=1, inverse=0, canon=1), ref["none"][1, 0], x)
    run_cross(dict(base, dif=0, inverse=1), ref["none"][0, 1], x)
