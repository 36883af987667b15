"""GPU: the heads of the bucket chains.  A chain that starts from nothing adds its first two entries as two affine points
(csrc/curve29.hpp add_affine_affine29, csrc/kernels_msm.hpp chain_head) in msm_accum_kernel, msm_accum_split_kernel and
msm_big_body; this runs the standalone MSMs on scalar sets crafted so that the first two entries of many buckets are a chosen
pair, and two proofs on top.

How a bucket is filled: a scalar d < 2^(c-1) has the single digit d (window 0), so it puts its point into bucket d - 1 and
nowhere else; the scalar 2^c - d has the digit -d there (the point is subtracted) and a carry, the digit +1 of window 1, which
lands in bucket 0.  The order of a bucket's entries is not fixed (the scatter hands out positions with atomics), so a pair that
has to meet in the head sits in a bucket of exactly two entries, and buckets of three repeat each composition many times.
Bucket 0 collects the carries and the fill: the bucket of many entries, oversized where the fill is long enough that lanes of
msm_big_body hold two entries and more.
"""
import random

import pytest

import coracle
import groth16 as g
from bn254 import Q, R, G1_GEN, G2_GEN, g1_add, g1_mul, g1_neg, g2_add, g2_mul, g2_neg

pytestmark = pytest.mark.gpu
MONT = 1 << 256
P_PUB, CSEED, TSEED = 73, 0x5A4B0001, 0x5A4B00FF


def _le(v):
    return int(v).to_bytes(32, "little")


def _enc1(P):
    return _le(P[0] * MONT % Q) + _le(P[1] * MONT % Q)


def _enc2(P):
    return b"".join(_le(x * MONT % Q) for x in (P[0][0], P[0][1], P[1][0], P[1][1]))


def _std(P):
    flat = [P[0], P[1]] if not isinstance(P[0], tuple) else [P[0][0], P[0][1], P[1][0], P[1][1]]
    return b"".join(_le(v) for v in flat)


NB = 6   # distinct base points; base NB + b is the negative of base b (another table point with the same x)
# what the first entries of a bucket are made of: (base, sign) with sign -1 = subtracted
RECIPES = [
    [(0, 1), (0, 1)],                       # the same point twice, exactly two entries: the head doubles
    [(1, -1), (1, -1)],                     # ... both subtracted
    [(0, 1), (0, -1)],                      # a point and its negative: the head gives infinity and the bucket stays empty
    [(2, 1), (NB + 2, 1)],                  # ... the negative as a table point of its own
    [(2, -1), (NB + 2, -1)],
    [(0, 1), (1, 1)], [(0, 1), (1, -1)], [(0, -1), (1, 1)], [(0, -1), (1, -1)],     # exactly two entries, every sign combination
    [(3, 1), (3, 1), (4, 1)],               # three entries: the doubling first, or in the loop
    [(3, 1), (3, -1), (4, 1)],              # a point and its negative followed by a third entry (or around it)
    [(5, -1), (NB + 5, -1), (1, -1)],
    [(4, 1)], [(4, -1)], [],                # one entry, none
    [(0, 1), (1, 1), (2, -1), (3, 1), (4, -1)],                                     # five: with four lanes per bucket one lane has two
    [(b % NB, 1 - 2 * (b % 3 == 1)) for b in range(9)],                             # nine: two or three entries per lane
    [(b % (2 * NB), 1 - 2 * (b % 4 == 2)) for b in range(41)],                      # many
]


def _bases(group):
    gen, mul, neg = (G1_GEN, g1_mul, g1_neg) if group == "g1" else (G2_GEN, g2_mul, g2_neg)
    pos = [mul(gen, 1000003 * b + 11) for b in range(NB)]
    return pos + [neg(P) for P in pos]


_BASES = {}


def bases(group):
    if group not in _BASES:
        _BASES[group] = _bases(group)
    return _BASES[group]


def crafted(c, n, rnd):
    """(base index, scalar) per point, n of them: the recipes over the buckets 1 .., the rest of n into bucket 0."""
    half = 1 << (c - 1)
    out = []
    d, k = 2, 0
    while d < half and d < 1500 and len(out) + 41 < n * 3 // 4:
        for base, sign in RECIPES[k % len(RECIPES)]:
            out.append((base, d if sign > 0 else (1 << c) - d))
        d += 1
        k += 1
    assert k >= 2 * len(RECIPES) or half <= 2 * len(RECIPES) + 2, (c, n, k)
    while len(out) < n:
        out.append((rnd.randrange(2 * NB), 1 if rnd.randrange(3) else (1 << c) - 1))
    rnd.shuffle(out)
    return out


# window bits, points: 2^10 .. 2^13 points; at c = 8 bucket 0 holds ~7000 entries (msm_big_kernel: 2048 lanes share it,
# three entries and more each); c <= 12: four lanes per bucket, c = 17: 2^16 buckets, two lanes per bucket, c = 19: 2^18 buckets, one
# lane per bucket (msm_accum_kernel itself)
CASES = [(8, 1 << 13), (9, 1 << 12), (10, 1 << 10), (11, 1 << 11), (12, 1 << 12), (17, 1 << 12), (19, 1 << 12)]


@pytest.mark.parametrize("group", ["g1", "g2"])
@pytest.mark.parametrize("c,n", CASES, ids=lambda v: str(v))
def test_crafted_chain_heads_through_the_standalone_msm(group, c, n, monkeypatch):
    import zkr_hip
    msm, omsm, enc, add, mul = ((zkr_hip.msm_g1, coracle.msm_g1, _enc1, g1_add, g1_mul) if group == "g1" else
                                (zkr_hip.msm_g2, coracle.msm_g2, _enc2, g2_add, g2_mul))
    monkeypatch.setenv("ZKR_MSM_C", str(c))
    B = bases(group)
    benc = [enc(P) for P in B]
    pairs = crafted(c, n, random.Random(100 * c + len(group)))
    assert len(pairs) == n
    pb = b"".join(benc[b] for b, _ in pairs)
    sb = b"".join(_le(s) for _, s in pairs)
    sums = [0] * len(B)
    for b, s in pairs:
        sums[b] += s
    want = None
    for b, P in enumerate(B):
        if sums[b] % R:
            want = add(want, mul(P, sums[b] % R))
    got = msm(pb, sb)
    assert got == (None if want is None else _std(want))
    assert got == omsm(pb, sb)


def test_buckets_of_pairs_only_cancel_to_infinity(monkeypatch):
    """Every bucket holds a point and its negative and nothing else: every head gives infinity, so does the MSM."""
    import zkr_hip
    c = 10
    monkeypatch.setenv("ZKR_MSM_C", str(c))
    B = bases("g1")
    pts, sc = [], []
    for d in range(2, 500):
        pts += [B[d % NB], B[NB + d % NB]]
        sc += [d, d]
    pb, sb = b"".join(_enc1(P) for P in pts), b"".join(_le(s) for s in sc)
    assert zkr_hip.msm_g1(pb, sb) is None and coracle.msm_g1(pb, sb) is None


def _threads():
    from bench import effective_host_cores
    return max(1, min(16, effective_host_cores()))


def test_tx_circuit_proof_equals_the_oracle_proof():
    """The tx circuit (2^17 constraints: 2^16 buckets, two lanes per bucket; its witness tables share supports, so chains meet
    infinity placeholders among their first entries)."""
    import zkr_hip
    from zkr_hip import rollup as n
    from test_rollup import as_inputs, scenario
    c = n.RollupCircuit()
    tox = g.toxic_from_seed(0x5A4B00F3)
    pkb, _ = zkr_hip.setup_r1cs_websnark(c.r1cs(), toxic=[tox[k] for k in ("t", "alfa", "beta", "gamma", "delta")])
    txs, _, _ = scenario(2, 6, 41, n_accounts=5)
    wb = c.calculate_witness(as_inputs(txs))
    rng = g.SplitMix64(2901)
    r, s = rng.fr(), rng.fr()
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    try:
        assert key.info()["domainSize"] == 1 << 17
        assert key.prove(wb, r, s) == coracle.prove_mt(pkb, wb, r, s, threads=_threads())
    finally:
        key.close()


def test_fused_batch_of_four_equals_the_oracle_proofs():
    import zkr_hip
    log_m = 14
    pkb, _ = zkr_hip.synth_websnark(log_m, P_PUB, CSEED, TSEED)
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    try:
        assert key.fuse() >= 4
        wits = [zkr_hip.synth_witness(log_m, P_PUB, CSEED, 2900 + j) for j in range(4)]
        rng = g.SplitMix64(2902)
        rs, ss = [rng.fr() for _ in wits], [rng.fr() for _ in wits]
        got = key.prove_batch(wits, rs, ss)
        for j in range(4):
            assert got[j] == coracle.prove_mt(pkb, wits[j], rs[j], ss[j], threads=_threads()), j
    finally:
        key.close()
