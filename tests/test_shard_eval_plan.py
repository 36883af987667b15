"""CPU: the split calcH of a sharded proof in evaluation form (csrc/zkr_prove.hip calc_h_split, phases 2-4) as index operations on
Python integers, with the pass model of tests/test_ntt_plan.py: P shards, shard j owning block j of every vector and taking columns
[j cols, (j + 1) cols) of every block in the cross passes.  After phase 4 -- written IN PLACE into every block -- block j must hold
the evaluations m A(g w^i) for the i of its range, in natural order."""
import random

import pytest

from bn254 import R
from test_ntt_plan import bitrev, make_tw, ntt_pass, run_ntt

TWL_LOG, TILE_LOG = 3, 4  # the scaled-down local twiddle table and tile of tests/test_ntt_plan.py


def cross_pass(blocks, L, klog, part, dif, inverse, tw, twl, out=None):
    """The top klog stages of a transform of 2^L points whose 2^klog blocks are separate buffers: shard `part` takes its columns of
    every block of `blocks` and stores them to the same places of `out` (default: in place).  Stages [L - klog, L) pair the same
    column of different blocks, so what the shard reads and writes is its columns alone -- asserted, not assumed."""
    P, Bk = 1 << klog, 1 << (L - klog)
    cols = Bk >> klog
    wlog = min(TILE_LOG - klog, cols.bit_length() - 1)
    flat = [v for b in blocks for v in b]
    ntt_pass(flat, L, L - klog, L, wlog, dif, inverse, tw, L, twl, TWL_LOG)
    # the same pass with every column that is not the shard's scrambled: the shard's columns must not notice
    rnd = random.Random(part)
    other = [v if part * cols <= c < (part + 1) * cols else rnd.randrange(R) for b in blocks for c, v in enumerate(b)]
    ntt_pass(other, L, L - klog, L, wlog, dif, inverse, tw, L, twl, TWL_LOG)
    out = blocks if out is None else out
    for r in range(P):
        for c in range(part * cols, (part + 1) * cols):
            assert flat[r * Bk + c] == other[r * Bk + c]
            out[r][c] = flat[r * Bk + c]


def coset_scale(block, Lb, klog, rev, tw):
    """PRE_COSET of a block of a larger transform (kernels_ntt.hpp NttPassArgs::pre_shift / pre_add): position gi of the block holds
    coefficient (bitrev(gi) << klog) | rev of the whole transform."""
    return [v * tw[(bitrev(gi, Lb) << klog) | rev] % R for gi, v in enumerate(block)]


@pytest.mark.parametrize("P", [2, 4])
def test_phases_2_to_4_leave_every_block_its_coset_evaluations(P):
    L = 6
    m, klog = 1 << L, P.bit_length() - 1
    Lb, Bk = L - klog, m >> klog
    tw, twl = make_tw(m), make_tw(1 << TWL_LOG)
    rnd = random.Random(0x5A4B + P)
    a = [rnd.randrange(R) for _ in range(m)]  # the QAP row sums on the domain, natural order (phase 1)
    # the oracle: coefficients by the inverse DFT, then m A(g w^i) term by term (g = w_2m, w = g^2)
    gen = tw[1]
    w = gen * gen % R
    minv = pow(m, R - 2, R)
    coef = [minv * sum(a[i] * pow(w, (-i * k) % m, R) for i in range(m)) % R for k in range(m)]
    want = [m * sum(ck * pow(gen * pow(w, i, R) % R, k, R) for k, ck in enumerate(coef)) % R for i in range(m)]

    va = [a[j * Bk:(j + 1) * Bk] for j in range(P)]
    ca = [[None] * Bk for _ in range(P)]
    # 2: CROSS top stages of the inverse transform, all blocks' va -> this shard's columns of every block's ca
    for j in range(P):
        cross_pass(va, L, klog, j, True, True, tw, twl, out=ca)
    assert all(v is not None for b in ca for v in b)  # the shards' columns tile every block
    # 3: the block's own stages (coefficients x m, bit-reversed), the coset factors with (klog, rev), the coset transform below its top stages
    for j in range(P):
        blk = ca[j]
        run_ntt(blk, Lb, True, True, tw, L, twl, TWL_LOG)
        blk = coset_scale(blk, Lb, klog, bitrev(j, klog), tw)
        run_ntt(blk, Lb, False, False, tw, L, twl, TWL_LOG)
        ca[j] = blk
    # 4: CROSS top stages of the coset transform, in place, shard after shard in either order
    for j in (range(P) if P == 2 else reversed(range(P))):
        cross_pass(ca, L, klog, j, False, False, tw, twl)
    for j in range(P):
        assert ca[j] == want[j * Bk:(j + 1) * Bk], (P, j)


def test_the_model_splits_what_the_whole_transform_does():
    """The same two transforms unsplit (tests/test_ntt_plan.py test_calc_h_pipeline_constants) give the same vector: the oracle above
    and the whole-domain route agree, so the split is compared with both."""
    L = 6
    m = 1 << L
    tw, twl = make_tw(m), make_tw(1 << TWL_LOG)
    rnd = random.Random(7)
    a = [rnd.randrange(R) for _ in range(m)]
    x = list(a)
    run_ntt(x, L, True, True, tw, L, twl, TWL_LOG)
    x = [x[p] * tw[bitrev(p, L)] % R for p in range(m)]
    run_ntt(x, L, False, False, tw, L, twl, TWL_LOG)
    for P in (2, 4):
        klog = P.bit_length() - 1
        Lb, Bk = L - klog, m >> klog
        ca = [[None] * Bk for _ in range(P)]
        va = [a[j * Bk:(j + 1) * Bk] for j in range(P)]
        for j in range(P):
            cross_pass(va, L, klog, j, True, True, tw, twl, out=ca)
        for j in range(P):
            blk = ca[j]
            run_ntt(blk, Lb, True, True, tw, L, twl, TWL_LOG)
            blk = coset_scale(blk, Lb, klog, bitrev(j, klog), tw)
            run_ntt(blk, Lb, False, False, tw, L, twl, TWL_LOG)
            ca[j] = blk
        for j in range(P):
            cross_pass(ca, L, klog, j, False, False, tw, twl)
        assert [v for b in ca for v in b] == x
