"""GPU: the MSM's oversized-bucket paths and window-edge geometry at the sizes where they switch on.

Part A proves skewed witnesses -- small integers, repeated digits, booleans, one spread value, scalars at the spreading
threshold -- with production-size keys and compares every proof with the C oracle.  Before proving, each family's bucket
occupancy is counted with the library's own rules (tests/msm_edge_model.py) to show that it reaches the path it is meant
for: more than BIG_CAP oversized buckets, several rounds of msm_big_body, buckets in the top size class, every spreading
class t.  Fused batches do the same with proofs that share one oversized-bucket list.  Part B runs the standalone MSM at
every window size ZKR_MSM_C accepts, with edge scalars, against sums formed with Python integers.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import coracle
import msm_edge_model as em
from bn254 import R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_PUB, CSEED, TSEED = 73, 0x5A4B0001, 0x5A4B00FF
BLIND_R, BLIND_S = 0x1D0C5E7A3B2F4E19A88C0D1E2F3A4B5C6D7E8F90A1B2C3D4E5F60718293A4B5C % R, 0x2E1F0D3C4B5A69788796A5B4C3D2E1F0 % R


def _threads():
    from bench import effective_host_cores
    return max(1, min(16, effective_host_cores()))


def _wb(w):
    return b"".join(int(x).to_bytes(32, "little") for x in w)


def _present(pkb):
    """Which scalar indices each witness table has a point for (the key drops points whose x is 0): A, B1, B2, C."""
    u32 = lambda o: int.from_bytes(pkb[o:o + 4], "little")
    n, p = u32(0), u32(4)
    pPA, pPB1, pPB2, pPC = (u32(12 + 4 * i) for i in (2, 3, 4, 5))
    buf = np.frombuffer(pkb, dtype=np.uint8)
    nz = lambda off, cnt, size, xb: buf[off:off + cnt * size].reshape(cnt, size)[:, :xb].any(axis=1)
    C = np.zeros(n, dtype=bool)
    C[p + 1:] = nz(pPC, n - p - 1, 64, 32)
    return dict(A=nz(pPA, n, 64, 32), B1=nz(pPB1, n, 64, 32), B2=nz(pPB2, n, 128, 64), C=C)


def _family(kind, n, c, K, rnd, small=1500, rep=1100):
    """Witness (w_0 = 1) of one skewed family, built for window bits c and K windows."""
    tmax = em.spread_tmax(c, K)
    if kind == "small_ints":
        w = [rnd.randint(1, small) for _ in range(n)]
    elif kind == "repeated_digit":
        unit = em.repeated_digit(c, K, 1)
        w = [rnd.randint(1, rep) * unit for _ in range(n)]
    elif kind == "booleans":
        w = [rnd.randrange(2) for _ in range(n)]
    elif kind == "one_value":
        w = [R - 1 - em.carry_chain(c, K)] * n
    elif kind == "threshold_mix":
        T, half = em.threshold(c, K), 1 << (c - 1)
        vals = [v for v in (T - 1, T, R - 2, R - 1, em.all_digits(c, K, half), em.all_digits(c, K, half + 1)) if v < R]
        per = max(tmax, 1)
        w = [vals[(i // per) % len(vals)] for i in range(n)]      # each value at a full run of t = 0 .. tmax - 1
    else:
        raise ValueError(kind)
    w[0] = 1
    return w


@pytest.fixture(scope="module", params=[18, 20], ids=lambda v: "m2^%d" % v)
def big_key(request):
    import zkr_hip
    log_m = request.param
    pkb, _ = zkr_hip.synth_websnark(log_m, P_PUB, CSEED, TSEED)
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    yield dict(log_m=log_m, pkb=pkb, key=key, info=key.info(), win=key.windows(), present=_present(pkb))
    key.close()


BIG_ROUNDS = em.BIG_CAP // em.BIG_SLOTS   # a full list takes 16 rounds of msm_big_body
FAMILIES = ["small_ints", "repeated_digit", "booleans", "one_value", "threshold_mix"]


@pytest.mark.parametrize("kind", FAMILIES)
def test_skewed_witness_at_production_size_equals_oracle(big_key, kind):
    """One proof per family at 2^18 and 2^20, bit-exact with coracle.prove_mt; the family's paths asserted first."""
    info, win, present = big_key["info"], big_key["win"], big_key["present"]
    n = info["nVars"]
    c, K = win["A"]
    tmax = em.spread_tmax(c, K)
    rnd = random.Random(sum(map(ord, kind)) * 100 + big_key["log_m"])
    w = _family(kind, n, c, K, rnd)
    reach = {}
    for t in ("A", "B1", "C") if kind in ("small_ints", "repeated_digit") else ("A", "C"):
        tc, tK = win[t]
        occ = em.occupancy(w, tc, tK, em.spread_tmax(tc, tK), present[t])
        reach[t] = em.paths(occ, em.big_threshold(info["pts" + t], tK, 1 << (tc - 1)))
    print(kind, "m = 2^%d" % big_key["log_m"], "c = %d" % c, reach)
    if kind == "small_ints":          # more than BIG_CAP oversized buckets in every witness table: hundreds stay in the accumulation
        assert all(reach[t]["over_cap"] > 0 for t in reach), reach
        assert reach["A"]["rounds"] == BIG_ROUNDS
    elif kind == "repeated_digit":    # more than BIG_CAP buckets of >= SIZE_BINS - 1 entries: some of the top class are over the cap
        assert all(reach[t]["top_class"] > em.BIG_CAP for t in reach), reach
    elif kind == "booleans":
        assert reach["A"]["over"] >= 1 and reach["C"]["over"] >= 1
    elif kind == "one_value":         # every index spread, every t
        assert w[1] >= em.threshold(c, K) and tmax > 1
        assert {em.spread_t(w[i], i, c, K, tmax) for i in range(1, n)} == set(range(tmax))
        assert reach["A"]["over"] >= 1
    elif kind == "threshold_mix":     # r - 1 and the threshold itself at every t
        for v in (R - 1, em.threshold(c, K)):
            assert {em.spread_t(w[i], i, c, K, tmax) for i in range(1, n) if w[i] == v} == set(range(tmax)), v
    wb = _wb(w)
    got = big_key["key"].prove(wb, BLIND_R, BLIND_S)
    assert got == coracle.prove_mt(big_key["pkb"], wb, BLIND_R, BLIND_S, threads=_threads())


# fused batch of 19 at 2^16 (fuse() = 16): zkr_prove_batch cuts it into two submits, each with one oversized-bucket list
FUSED_ORDER = ["small_ints", "small_ints", "repeated_digit", "synth", "small_ints", "one_value", "small_ints", "threshold_mix",
               "small_ints", "small_ints",
               "small_ints", "booleans", "small_ints", "repeated_digit", "synth", "small_ints", "small_ints", "small_ints",
               "threshold_mix"]


def test_fused_batches_share_one_oversized_list_without_leaking():
    """19 skewed and satisfying witnesses at 2^16 through prove_batch and prove_batch_device: the groups' oversized buckets
    together overflow BIG_CAP (asserted from the occupancy, with the fused threshold), and every proof equals its own
    single proof; a sample equals the oracle."""
    import torch
    import zkr_hip
    log_m = 16
    pkb, _ = zkr_hip.synth_websnark(log_m, P_PUB, CSEED, TSEED)
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    try:
        info, win, present = key.info(), key.windows(), _present(pkb)
        assert key.fuse() == em.MAX_FUSE
        n = info["nVars"]
        c, K = win["A"]
        rnd = random.Random(1616)
        wits, ws = [], []
        for j, kind in enumerate(FUSED_ORDER):
            if kind == "synth":
                wb = zkr_hip.synth_witness(log_m, P_PUB, CSEED, 4400 + j)
                ws.append(None)
            else:
                w = _family(kind, n, c, K, rnd, small=200, rep=60)
                ws.append(w)
                wb = _wb(w)
            wits.append(wb)
        groups = em.group_sizes(len(wits), key.fuse())
        assert sum(groups) == len(wits) and max(groups) <= key.fuse() and len(groups) == 2
        at = 0
        for nbat in groups:
            for t in ("A", "C"):
                tc, tK = win[t]
                thr = em.big_threshold(info["pts" + t], tK, 1 << (tc - 1), nbat)
                over = 0
                for j in range(nbat):
                    w = ws[at + j]
                    if w is not None:   # satisfying witnesses only add to it
                        occ = em.occupancy(w, tc, tK, em.spread_tmax(tc, tK), present[t], base_index=j * n)
                        over += em.paths(occ, thr)["over"]
                print("group of %d, table %s: threshold %d, %d oversized buckets" % (nbat, t, thr, over))
                assert over > em.BIG_CAP, (nbat, t, over)
            at += nbat
        rng = random.Random(77)
        rs, ss = [rng.randrange(R) for _ in wits], [rng.randrange(R) for _ in wits]
        host = key.prove_batch(wits, rs, ss)
        dw = [torch.frombuffer(bytearray(w), dtype=torch.uint8).cuda() for w in wits]
        dev = key.prove_batch_device([t.data_ptr() for t in dw], rs, ss)
        single = [key.prove(w, r, s) for w, r, s in zip(wits, rs, ss)]
        for j in range(len(wits)):
            assert host[j] == single[j] == dev[j], (j, FUSED_ORDER[j])
        for j in (0, 2, 5, 7, 11, 14):
            assert single[j] == coracle.prove_mt(pkb, wits[j], rs[j], ss[j], threads=_threads()), (j, FUSED_ORDER[j])
    finally:
        key.close()


# ---------------------------------------------------------------- B: every window size through the standalone MSM
_WINDOW_CHILD = r"""
import os, random, sys
sys.path[:0] = %r
import coracle, zkr_hip
import msm_edge_model as em
from bn254 import Q, R, G1_GEN, G2_GEN, g1_add, g1_mul, g2_add, g2_mul
MONT = 1 << 256
le = lambda v: int(v).to_bytes(32, "little")
def enc1(P):
    return le(0) + le(MONT %% Q) if P is None else le(P[0] * MONT %% Q) + le(P[1] * MONT %% Q)
def enc2(P):
    return le(0) * 2 + le(MONT %% Q) + le(0) if P is None else b"".join(le(x * MONT %% Q) for x in (P[0][0], P[0][1], P[1][0], P[1][1]))
def std1(P):
    return le(P[0]) + le(P[1])
def std2(P):
    return b"".join(le(x) for x in (P[0][0], P[0][1], P[1][0], P[1][1]))
GROUPS = dict(g1=(zkr_hip.msm_g1, coracle.msm_g1, G1_GEN, g1_add, g1_mul, enc1, std1, 16),
              g2=(zkr_hip.msm_g2, coracle.msm_g2, G2_GEN, g2_add, g2_mul, enc2, std2, 8))
cases = 0
for group, cs in %r:
    msm, omsm, gen, add, mul, enc, std, D = GROUPS[group]
    # D distinct bases k G (order r: the spreading needs it), one of them the point at infinity (no rank)
    bases = [None if b == D // 2 else mul(gen, 1000003 * b + 7) for b in range(D)]
    benc = [enc(P) for P in bases]
    for c in cs:
        os.environ["ZKR_MSM_C"] = str(c)
        K = em.windows(c)
        tmax = em.spread_tmax(c, K)
        rnd = random.Random(1000 * c + D)
        per_pt = (D - 1) / D
        n_chunks = int(1.3 * em.plan(1, c)["nR"] * em.SORT_CHUNK_RECORDS / K / per_pt) + D
        runs = [("edges", max(tmax + 2, 700)), ("edges", n_chunks)]
        if 3 <= c <= 8:
            runs.append(("big", 3000))
        for shape, n in runs:
            if shape == "edges":
                sc = em.edge_vector(c, K, n, rnd)
            else:     # repeated digits: K - 1 entries per scalar in bucket 0 (bucket 1 for a tenth)
                sc = [em.repeated_digit(c, K, 2 if i %% 10 == 3 else 1) for i in range(n)]
                occ = em.occupancy(sc, c, K, tmax, [i %% D != D // 2 for i in range(n)])
                np_ = sum(1 for i in range(n) if i %% D != D // 2)
                assert em.paths(occ, em.big_threshold(np_, K, 1 << (c - 1)))["over"] >= 1, (group, c)
            if shape == "edges" and n == n_chunks:
                assert em.plan(sum(1 for i in range(n) if i %% D != D // 2), c)["J"] >= 2, (group, c)   # several sort chunks
            # words >= r where they fit in 256 bits: ingest reduces them
            raw = [s + R if i %% 29 == 4 and s + R < MONT else (MONT - 1 if i %% 31 == 9 else s) for i, s in enumerate(sc)]
            red = [x %% R for x in raw]
            want = None
            sums = [0] * D
            for i, s in enumerate(red):
                sums[i %% D] += s
            for b in range(D):
                if bases[b] is not None and sums[b] %% R:
                    want = add(want, mul(bases[b], sums[b] %% R))
            pb = b"".join(benc[i %% D] for i in range(n))
            got = msm(pb, b"".join(le(x) for x in raw))
            assert got == (None if want is None else std(want)), (group, c, shape, n)
            if n <= 5000:
                assert got == omsm(pb, b"".join(le(x) for x in red)), (group, c, shape, n)
            cases += 1
print("windows ok", cases)
"""

WINDOW_GROUPS = [
    [("g1", [2, 3, 4, 5, 6])],
    [("g1", [7, 8, 9, 10, 11, 12])],
    [("g1", [13, 14, 15, 16, 17])],
    [("g1", [18, 19, 20])],
    [("g1", [21, 22])],
    [("g2", [2, 3, 5, 16])],
    [("g2", [18, 21, 22])],
]


@pytest.mark.parametrize("spec", WINDOW_GROUPS, ids=lambda s: ",".join("%s:c=%s" % (g, "/".join(map(str, cs))) for g, cs in s))
def test_every_window_size_through_the_standalone_msm(spec):
    """ZKR_MSM_C = 2 .. 22 for G1 and 2, 3, 5, 16, 18, 21, 22 for G2, each group in a fresh process: edge scalars (the spreading
    threshold +- 1, r - 1 at indices of class tmax - 1, all-half digits, carry chains, zeros, words >= r) over tmax + 1 or more
    entries, vectors long enough for several sort chunks, and oversized buckets at the narrow windows; the result equals the
    sum formed with Python integers (and the C oracle on the shorter vectors)."""
    env = dict(os.environ)
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "simple-zk-rollups_amd", "python")] + sys.path
    out = subprocess.run([sys.executable, "-c", _WINDOW_CHILD % (paths, spec)], env=env, capture_output=True, text=True, timeout=900)
    want = sum(len(cs) * 2 + sum(1 for c in cs if 3 <= c <= 8) for _, cs in spec)
    assert out.returncode == 0 and ("windows ok %d" % want) in out.stdout, out.stderr[-3000:]
