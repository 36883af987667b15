"""What ONE launch sequence of the NTT drivers (csrc/zkr_prove.hip run_ntt / run_ntt_cross, through zkr_selftest_ntt) must leave in
memory, mode by mode, as plain integers in terms of the oracle's transform (groth16.ntt for small sizes, coracle.ntt for large
ones; roots as groth16.root_of_unity gives them).  Shared by tests/test_ntt_cases_cpu.py (these formulas against an O(n^2)
evaluation of the definitions and against the pass model of tests/test_ntt_plan.py) and tests/test_gpu_ntt_modes.py (the device
against these formulas).  Not a test module.  Nothing here calls the product.

With br = bit reversal over L bits, n = 2^L, F = NTT(X) (F[i] = sum_k X[k] w_n^(i k)), g = w_{2^(tlog+1)}, MONT = 2^256:
  DIF: natural in, X = in, out[br(i)] = F[i] (forward) or F[-i mod n] = n iNTT(X)[i] (inverse: unscaled);
  DIT: bit-reversed in, X[i] = in[br(i)], natural out: out[i] = F[i] or F[-i mod n];
  PRE_COSET: position gi of the input is first multiplied by g^(((br(gi) << shift) | add) << (tlog - L - shift));
  PRE_MUL: position gi is first replaced by in0[gi] in1[gi] / MONT;
  nbat vectors end to end and the second transform of a pair: independent transforms;
  an output range: only [want_lo, want_lo + want_n) of (each transform's) output is defined;
  cross: stages [L - klog, L) of the pass model (test_ntt_plan.ntt_pass), columns [col_lo, col_lo + col_n) of every row block."""
import functools

import numpy as np

import coracle
import groth16 as g
from bn254 import R
from test_ntt_plan import bitrev, make_tw, ntt_pass

MONT_INV = pow(1 << 256, R - 2, R)
TWL_LOG, TILE_LOG = 10, 11          # csrc/kernels_ntt.hpp
PRE_NONE, PRE_COSET, PRE_MUL = 0, 1, 2
ORACLE_SMALL_LOG = 8                # up to here the Python oracle, above it the C one
FILL = 0xA5                         # what a test puts into `out` before the run


def pack(words):
    return b"".join(int(v).to_bytes(32, "little") for v in words)


def unpack(data):
    return [int.from_bytes(data[i:i + 32], "little") for i in range(0, len(data), 32)]


@functools.lru_cache(maxsize=None)
def bitrev_perm(L):
    """numpy: p[i] = br(i) over L bits"""
    p = np.zeros(1 << L, dtype=np.int64)
    for b in range(L):
        p |= ((np.arange(1 << L, dtype=np.int64) >> b) & 1) << (L - 1 - b)
    return p


def oracle_ntt(x):
    """the oracle's forward transform of a list of integers"""
    if len(x) <= 1 << ORACLE_SMALL_LOG:
        return g.ntt(x)
    return unpack(coracle.ntt(pack(x)))


def coset_exponent(gi, L, tlog, shift, add):
    return ((bitrev(gi, L) << shift) | add) << (tlog - L - shift)


def pre_apply(pre, in0, in1, L, tlog=None, shift=0, add=0):
    """what the first pass makes of one transform's input before its butterflies"""
    if pre == PRE_NONE:
        return list(in0)
    if pre == PRE_MUL:
        return [a * b * MONT_INV % R for a, b in zip(in0, in1)]
    gen = g.root_of_unity(1 << (tlog + 1))
    if shift == 0 and add == 0 and tlog == L:       # the whole transform: one table of powers instead of n pow() calls
        tw = make_tw(1 << L)
        return [v * tw[bitrev(gi, L)] % R for gi, v in enumerate(in0)]
    return [v * pow(gen, coset_exponent(gi, L, tlog, shift, add), R) % R for gi, v in enumerate(in0)]


def transform(x, L, dif, inverse):
    """one transform's raw output from its (pre-processed) input, by the oracle"""
    n = 1 << L
    br = bitrev_perm(L).tolist()
    X = x if dif else [x[br[i]] for i in range(n)]
    F = oracle_ntt(X)
    if inverse:
        F = [F[(n - i) % n] for i in range(n)]
    return [F[br[p]] for p in range(n)] if dif else F


_last_forward = [None, None]  # the last large forward transform: the directions of one size share it


def transform_bytes(data, L, dif, inverse):
    """the same for PRE_NONE on bytes, with numpy row permutations and the C oracle: what a 2^21 transform can afford"""
    n = 1 << L
    br = bitrev_perm(L)
    rows = np.frombuffer(data, dtype=np.uint8).reshape(n, 32)
    X = (rows if dif else rows[br]).tobytes()
    if _last_forward[0] != X:
        _last_forward[:] = [X, coracle.ntt(X)]
    F = np.frombuffer(_last_forward[1], dtype=np.uint8).reshape(n, 32)
    if inverse:
        F = F[(n - np.arange(n)) % n]
    return (F[br] if dif else F).tobytes()


def plain_expected(desc, in0, in1=None):
    """run_ntt: the whole raw output for the nbat vectors of `in0` (and `in1`), lists of integers end to end"""
    L, nbat = desc["logn"], desc.get("nbat", 1)
    shift, add = desc.get("coset_shift", 0), desc.get("coset_add", 0)
    tlog = desc.get("tlog", L + shift)
    n, out = 1 << L, []
    for b in range(nbat):
        x = pre_apply(desc.get("pre", 0), in0[b * n:(b + 1) * n], in1[b * n:(b + 1) * n] if in1 is not None else None, L, tlog, shift, add)
        out += transform(x, L, bool(desc["dif"]), bool(desc["inverse"]))
    return out


def wanted(desc):
    """the positions of one transform's output that the run defines"""
    if desc.get("want_n", 0):
        return range(desc["want_lo"], desc["want_lo"] + desc["want_n"])
    return range(1 << desc["logn"])


def check_plain(desc, got, in0, in1=None, in0_b=None, in1_b=None):
    """`got`: the vectors after the run (zkr_hip.selftest_ntt) as bytes.  The defined part of the output equals plain_expected byte
    for byte (the last pass stores canonical residues); an out-of-place run leaves its inputs as they were, an in-place one the
    second operand of its products."""
    L, nbat, n = desc["logn"], desc.get("nbat", 1), 1 << desc["logn"]
    in_place = bool(desc.get("in_place", 0))
    sides = [("", in0, in1)] + ([("_b", in0_b, in1_b)] if desc.get("pair", 0) else [])
    assert set(got) == {nm + s for s, _, i1 in sides for nm in ["in0"] + (["in1"] if i1 is not None else []) + ([] if in_place else ["out"])}
    for s, a, b in sides:
        want = plain_expected(desc, a, b)
        have = got["in0" + s] if in_place else got["out" + s]
        assert len(have) == 32 * nbat * n
        rng = wanted(desc)
        for t in range(nbat):
            lo, hi = t * n + rng[0], t * n + rng[-1] + 1
            if have[32 * lo:32 * hi] != pack(want[lo:hi]):
                first = next(p for p in range(lo, hi) if have[32 * p:32 * p + 32] != pack(want[p:p + 1]))
                raise AssertionError("%r: transform %d of side %r differs first at position %d of its output" % (desc, t, s or "a", first - t * n))
        if not in_place:
            assert got["in0" + s] == pack(a), "the run changed its input"
        if b is not None:
            assert got["in1" + s] == pack(b), "the run changed its second operand"


# ---------------------------------------------------------------------------------------------------------------- cross passes
@functools.lru_cache(maxsize=None)
def _tables(tlog):
    return make_tw(1 << tlog), make_tw(1 << TWL_LOG)


def cross_expected(x, L, klog, dif, inverse, tlog=None):
    """Stages [L - klog, L) of a transform of 2^L points on the whole vector `x` (the 2^klog row blocks end to end, already
    pre-processed): the pass model of tests/test_ntt_plan.py with the device's local table.  The tile width does not change what
    the stages compute, so the model runs with one that suits it."""
    tlog = L if tlog is None else tlog
    tw, twl = _tables(tlog)
    y = list(x)
    lo = L - klog
    ntt_pass(y, L, lo, L, min(lo, TILE_LOG - klog), dif, inverse, tw, tlog, twl, TWL_LOG)
    return y


def cross_wlog(klog, col_n):
    """log2 of the tile width run_ntt_cross picks (zkr_prove.hip ntt_cross_wlog)"""
    wlog = TILE_LOG - klog
    while (1 << wlog) > col_n:
        wlog -= 1
    return wlog


def cross_vectors(desc, full):
    """the bytes zkr_selftest_ntt takes for an input whose whole row blocks are `full`: the blocks end to end, or this shard's
    columns of each when in_sub says the buffers are local"""
    Bk = 1 << (desc["logn"] - desc["klog"])
    if not desc.get("in_sub", 0):
        return pack(full)
    lo, cn = desc["col_lo"], desc["col_n"]
    return pack([v for r in range(1 << desc["klog"]) for v in full[r * Bk + lo:r * Bk + lo + cn]])


def check_cross(desc, got, want_full, in0_full, in1_full=None):
    """want_full: cross_expected of the (pre-processed) whole input.  Columns [col_lo, col_lo + col_n) of every row block of the
    output equal it -- byte for byte when canon, else mod r with every stored word below 3 r; every other column the output
    buffers hold is what it was (FILL, or the input of an in-place run); inputs of an out-of-place run are unchanged."""
    L, klog = desc["logn"], desc["klog"]
    rows, Bk = 1 << klog, 1 << (L - klog)
    lo, cn = desc["col_lo"], desc["col_n"]
    in_place = bool(desc.get("in_place", 0))
    out_sub = desc.get("out_sub", 0)
    have = got["in0"] if in_place else got["out"]
    width = cn if out_sub else Bk
    assert len(have) == 32 * rows * width
    for r in range(rows):
        for c in range(lo, lo + cn):
            at = 32 * (r * width + c - out_sub)
            w = int.from_bytes(have[at:at + 32], "little")
            e = want_full[r * Bk + c]
            if desc.get("canon", 0):
                assert w == e, (desc, r, c)
            else:
                assert w < 3 * R and w % R == e, (desc, r, c)
    if not out_sub:                                  # whole blocks: the other shards' columns
        before = pack(in0_full) if in_place else bytes([FILL]) * len(have)
        for r in range(rows):
            a, b = 32 * r * Bk, 32 * (r * Bk + lo)
            assert have[a:b] == before[a:b], ("columns in front of the shard's changed", desc, r)
            a, b = 32 * (r * Bk + lo + cn), 32 * (r + 1) * Bk
            assert have[a:b] == before[a:b], ("columns behind the shard's changed", desc, r)
    if not in_place:
        assert got["in0"] == cross_vectors(desc, in0_full), "the run changed its input"
    if in1_full is not None:
        assert got["in1"] == cross_vectors(desc, in1_full), "the run changed its second operand"
