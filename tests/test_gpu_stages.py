"""GPU parity of each stage against the CPU oracle, through the C ABI (include/zkr.h)."""
import os
import random

import pytest

import coracle
import groth16 as g
from bn254 import Q, R, G1_GEN, G2_GEN, g1_mul, g2_mul, g1_add, g2_add

pytestmark = pytest.mark.gpu
MONT = 1 << 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _le(v):
    return int(v).to_bytes(32, "little")


def _g1_bytes(P):  # Montgomery wire form; None -> snarkjs zero [0,1,0]
    if P is None:
        return _le(0) + _le(MONT % Q)
    return _le(P[0] * MONT % Q) + _le(P[1] * MONT % Q)


def _g2_bytes(P):
    if P is None:
        return _le(0) + _le(0) + _le(MONT % Q) + _le(0)
    return b"".join(_le(c * MONT % Q) for c in (P[0][0], P[0][1], P[1][0], P[1][1]))


def test_device_product_forms_equal_the_host_recursion_limb_for_limb():
    """The hot path's Montgomery products run on the device as one hand-written instruction sequence per form
    (csrc/field29_asm.hpp); their definition is the C++ column recursion of csrc/field29.hpp, which the host build runs
    (and tests/test_host_arith.py checks against the integers).  Same raw limbs in, same raw limbs out, for operands with
    every limb at 2^29 - 1, sparse limbs and random ones, both fields, all four forms -- and for factors without their carry sweep
    (limbs up to 2^30 - 1 and 3 * 2^29 - 1) at their ceilings, in the weight patterns the group law instantiates."""
    import ctypes
    import os
    import random
    import zkr_hip
    from test_host_arith import SHIM, _raw_records, _raw_records_loose, raw_forms_host
    assert os.path.exists(SHIM), "host arithmetic shim not built (run __graft_entry__.build())"
    host = ctypes.CDLL(SHIM)
    recs = _raw_records(random.Random(61), 3000)
    for field in (0, 1):
        for form in range(4):
            assert zkr_hip.selftest_f29_forms(field, form, recs) == raw_forms_host(host, field, form, recs), (field, form)
    for (form, weights), loose in _raw_records_loose(random.Random(62), 400).items():
        for field in (0, 1):
            assert zkr_hip.selftest_f29_forms(field, form, loose) == raw_forms_host(host, field, form, loose), (field, form, weights)


def test_fq_mul_microbench_runs():
    import zkr_hip
    assert zkr_hip.bench_fq_mul() > 0.1  # G mul/s


@pytest.mark.parametrize("logn", [1, 2, 5, 10, 11, 12, 14])
def test_ntt_matches_oracle(logn):
    import zkr_hip
    rnd = random.Random(logn)
    n = 1 << logn
    v = [rnd.randrange(R) for _ in range(n)]
    v[0] = R - 1
    data = b"".join(_le(x) for x in v)
    assert zkr_hip.ntt(data) == coracle.ntt(data)
    assert zkr_hip.ntt(data, inverse=True) == coracle.ntt(data, inverse=True)


@pytest.mark.parametrize("logn", [11, 13, 16])
def test_ntt_extreme_inputs_match_oracle(logn):
    """The butterflies keep lazily reduced values (kernels_ntt.hpp: a DIF pair of stages quadruples one of its outputs before
    the quotient-estimate reduction): vectors whose entries are all r - 1, only 0 and r - 1, and values whose 29-bit limbs are
    all ones drive every intermediate to the top of its bound.  zkr_ntt launches DIF passes only, forward and inverse; the DIT
    bounds (sums grow by up to 4 half-moduli per stage of a DIT pass) are driven by
    tests/test_gpu_ntt_modes.py::test_structured_inputs_in_every_direction.
    Sizes: one full-tile pass (2^11), a short strided pass in front of it (2^13), two long passes (2^16)."""
    import zkr_hip
    rnd = random.Random(1000 + logn)
    n = 1 << logn
    ones29 = ((1 << 253) - 1) % R
    cases = [[R - 1] * n,
             [(R - 1) if rnd.random() < 0.5 else 0 for _ in range(n)],
             [rnd.choice((R - 1, R - 2, ones29, (1 << 232) - 1, 1, 0)) for _ in range(n)]]
    for v in cases:
        data = b"".join(_le(x) for x in v)
        assert zkr_hip.ntt(data) == coracle.ntt(data)
        assert zkr_hip.ntt(data, inverse=True) == coracle.ntt(data, inverse=True)


def test_ntt_reduces_words_above_r_first():
    """Words of 2^256 - 1, r, r + 5 are taken mod r before the transform (the passes state bounds on what they load)."""
    import zkr_hip
    rnd = random.Random(5)
    n = 64
    raw = [(1 << 256) - 1, R, R + 5, 3 * R + 1] + [rnd.randrange(1 << 256) for _ in range(n - 4)]
    a = zkr_hip.ntt(b"".join(_le(v) for v in raw), False)
    b = zkr_hip.ntt(b"".join(_le(v % R) for v in raw), False)
    assert a == b
    assert all(int.from_bytes(a[32 * i:32 * i + 32], "little") < R for i in range(n))


def test_ntt_roundtrip_and_linearity_2_20():
    import zkr_hip
    rnd = random.Random(20)
    n = 1 << 20
    a = [rnd.randrange(R) for _ in range(n)]
    da = b"".join(_le(x) for x in a)
    fa = zkr_hip.ntt(da)
    assert zkr_hip.ntt(fa, inverse=True) == da
    # X[0] = sum a_i ; x[0] of inverse = mean
    assert int.from_bytes(fa[:32], "little") == sum(a) % R
    # spot check against the C oracle (full transform)
    assert fa == coracle.ntt(da)


def _points_g1(n, rnd, with_inf=True):
    pts, P = [], G1_GEN
    for i in range(n):
        pts.append(None if with_inf and i % 7 == 3 else P)
        P = g1_add(P, G1_GEN) if i % 5 else g1_mul(P, 3)
    return pts


@pytest.mark.parametrize("n", [1, 2, 65, 1000, 20000])
def test_msm_g1_matches_oracle(n):
    import zkr_hip
    rnd = random.Random(n)
    pts = _points_g1(min(n, 300), rnd)
    pts = [pts[i % len(pts)] for i in range(n)]  # duplicates included on purpose
    sc = [rnd.randrange(R) for _ in range(n)]
    for i in range(0, n, 11):
        sc[i] = rnd.choice([0, 1, 1, 2, R - 1, (1 << 64) - 1, 1 << 253])
    pb = b"".join(_g1_bytes(P) for P in pts)
    sb = b"".join(_le(x) for x in sc)
    assert zkr_hip.msm_g1(pb, sb) == coracle.msm_g1(pb, sb)


def test_msm_g1_all_ones_goes_through_big_bucket_path():
    import zkr_hip
    n = 6000
    pts = _points_g1(200, None, with_inf=False)
    pts = [pts[i % 200] for i in range(n)]
    sc = [1] * n
    sc[5] = 0
    pb = b"".join(_g1_bytes(P) for P in pts)
    sb = b"".join(_le(x) for x in sc)
    assert zkr_hip.msm_g1(pb, sb) == coracle.msm_g1(pb, sb)


def test_msm_g1_cancels_to_infinity():
    import zkr_hip
    P = g1_mul(G1_GEN, 12345)
    pb = _g1_bytes(P) * 2
    sb = _le(5) + _le(R - 5)
    assert zkr_hip.msm_g1(pb, sb) is None
    assert coracle.msm_g1(pb, sb) is None


@pytest.mark.parametrize("n", [1, 3, 500, 5000])
def test_msm_g2_matches_oracle(n):
    import zkr_hip
    rnd = random.Random(n)
    base = [g2_mul(G2_GEN, rnd.randrange(1, R)) for _ in range(min(n, 40))]
    pts = [None if i % 9 == 4 else base[i % len(base)] for i in range(n)]
    sc = [rnd.randrange(R) for _ in range(n)]
    for i in range(0, n, 13):
        sc[i] = rnd.choice([0, 1, R - 1, 7])
    pb = b"".join(_g2_bytes(P) for P in pts)
    sb = b"".join(_le(x) for x in sc)
    assert zkr_hip.msm_g2(pb, sb) == coracle.msm_g2(pb, sb)


def test_reference_held_points_through_the_hip_msm():
    """The only group elements the reference tree itself holds -- the 80 G1 + 6 G2 verifying-key constants of
    contracts/contracts/TxVerifier.sol:176-257 and WithdrawVerifier.sol (tests/golden/verifier_points.json, extracted by
    tests/golden/make_verifier_points.py) -- as the base points of zkr_msm_g1 / zkr_msm_g2 with seeded random scalars: the HIP MSM,
    the C oracle and a sum formed with Python integers (oracle/bn254.py) agree.  Proof bytes stay unpinned by the reference
    (withdrawverifier.test.ts:27-37 checks validity only); this pins the MSM on points that are the reference's own."""
    import json
    import zkr_hip
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "verifier_points.json")))
    rnd = random.Random(0x5A4B)
    n1 = n2 = 0
    for name, c in fx["contracts"].items():
        g1 = [(int(x), int(y)) for _, (x, y) in sorted(c["g1"].items())]
        g2 = [((int(x0), int(x1)), (int(y0), int(y1))) for _, ((x1, x0), (y1, y0)) in sorted(c["g2"].items())]  # Solidity order [im, re]
        n1 += len(g1)
        n2 += len(g2)
        for pts, to_bytes, msm, omsm, add, mul in ((g1, _g1_bytes, zkr_hip.msm_g1, coracle.msm_g1, g1_add, g1_mul),
                                                   (g2, _g2_bytes, zkr_hip.msm_g2, coracle.msm_g2, g2_add, g2_mul)):
            sc = [rnd.randrange(R) for _ in pts]
            sc[0], sc[-1] = R - 1, 1
            pb, sb = b"".join(to_bytes(P) for P in pts), b"".join(_le(x) for x in sc)
            got = msm(pb, sb)
            assert got == omsm(pb, sb), name
            want = None
            for P, k in zip(pts, sc):
                want = add(want, mul(P, k))
            flat = [want[0], want[1]] if not isinstance(want[0], tuple) else [want[0][0], want[0][1], want[1][0], want[1][1]]
            assert got == b"".join(_le(v) for v in flat), name       # std affine out (include/zkr.h)
            # the same points many times over (a table long enough for the windowed path: 2^12 points), scalars that sum per point
            reps = 4096 // len(pts) + 1
            big_sc = [[rnd.randrange(R) for _ in range(reps)] for _ in pts]
            pb2 = b"".join(to_bytes(P) for P in pts for _ in range(reps))
            sb2 = b"".join(_le(x) for row in big_sc for x in row)
            want2 = None
            for P, row in zip(pts, big_sc):
                want2 = add(want2, mul(P, sum(row) % R))
            flat2 = [want2[0], want2[1]] if not isinstance(want2[0], tuple) else [want2[0][0], want2[0][1], want2[1][0], want2[1][1]]
            assert msm(pb2, sb2) == b"".join(_le(v) for v in flat2) == omsm(pb2, sb2), name
    assert (n1, n2) == (80, 6)


def test_calc_h_and_prove_small_key_from_python_oracle(small_case):
    import zkr_hip
    c = small_case
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    info = key.info()
    assert (info["nVars"], info["nPublic"], info["domainSize"]) == (c["pk"]["nVars"], 7, 128)
    h = g.calc_h_websnark(c["pk"], c["w"])
    assert key.calc_h(c["wb"]) == b"".join(_le(x) for x in h)
    proof = key.prove(c["wb"], c["r"], c["s"])
    expect = g.proof_from_toxic(c["circ"], c["tox"], c["w"], c["r"], c["s"])
    assert proof == g.proof_bytes(expect)           # bit-exact with the closed form
    assert proof == coracle.prove(c["pkb"], c["wb"], c["r"], c["s"])
    pj = zkr_hip.proof_json_from_bytes(proof)
    pts = dict(pi_a=(int(pj["pi_a"][0]), int(pj["pi_a"][1])),
               pi_b=((int(pj["pi_b"][0][0]), int(pj["pi_b"][0][1])), (int(pj["pi_b"][1][0]), int(pj["pi_b"][1][1]))),
               pi_c=(int(pj["pi_c"][0]), int(pj["pi_c"][1])))
    assert g.is_valid(c["vk"], pts, c["w"][1:8])    # TxVerifier.sol:258-276 equation
    # unsatisfied witness: same (invalid) proof as the reference algorithm yields
    w2 = list(c["w"])
    w2[20] = (w2[20] + 5) % R
    wb2 = g.binarify_witness(w2)
    assert key.prove(wb2, c["r"], c["s"]) == coracle.prove(c["pkb"], wb2, c["r"], c["s"])
    # random blinding: valid but different each call
    p1, p2 = key.prove(c["wb"]), key.prove(c["wb"])
    assert p1 != p2


def test_error_paths(small_case):
    import zkr_hip
    c = small_case
    with pytest.raises(zkr_hip.ZkrError):
        zkr_hip.ProvingKey.load_websnark(c["pkb"][:-1])
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    with pytest.raises(zkr_hip.ZkrError):
        key.prove(c["wb"][:-32], 1, 2)
    with pytest.raises(zkr_hip.ZkrError):
        key.prove(c["wb"], R, 2)
    # malformed section pointers must be refused before anything is read through them
    pk = bytearray(c["pkb"])
    def with_u32(off, v):
        b = bytearray(pk)
        b[off:off + 4] = int(v).to_bytes(4, "little")
        return bytes(b)
    for bad in (with_u32(16, len(pk) + 4096),        # polsB pointer past the buffer (the polsA scan would run off the end)
                with_u32(16, 0xFFFFFFF0),
                with_u32(16, 100),                   # before the fixed header
                with_u32(20, len(pk) + 64),          # pointsA pointer past the buffer
                with_u32(4, 0xFFFFFFFF),             # nPublic + 1 wraps around
                with_u32(12, 484)):                  # polsA pointer
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.ProvingKey.load_websnark(bad)
        assert e.value.code == -2


@pytest.mark.parametrize("log_m,p", [(6, 5), (10, 7), (13, 73)])
def test_synth_generator_and_device_setup_match_oracle(log_m, p):
    """product-side generator + device fixed-base setup == oracle generator + setup, byte for byte"""
    import zkr_hip
    pkb, wb = zkr_hip.synth_websnark(log_m, p, 0x5A4B0001, 0x5A4B00FF)
    if log_m <= 10:
        circ = g.synth_circuit(1 << log_m, p, 0x5A4B0001)
        assert g.binarify_witness(circ["witness"]) == wb
        pk, _ = g.setup(circ, g.toxic_from_seed(0x5A4B00FF))
        assert g.binarify_proving_key(g.to_json_key(pk)) == pkb
    rng = g.SplitMix64(log_m)
    r, s = rng.fr(), rng.fr()
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    proof = key.prove(wb, r, s)
    assert proof == coracle.prove(pkb, wb, r, s)
    # the arena-built key (no websnark binary) gives the same proof
    key2, wb2, aux = zkr_hip.ProvingKey.synth(log_m, p, 0x5A4B0001, 0x5A4B00FF)
    assert wb2 == wb
    assert key2.prove(wb, r, s) == proof
    # a replica adopted from the arena bytes proves identically
    import torch
    ptr, n = key2.arena()
    from zkr_hip.batch import _tensor_from_ptr
    replica_mem = _tensor_from_ptr(ptr, n, 0).clone()
    key3 = zkr_hip.ProvingKey.adopt_arena(replica_mem.data_ptr(), n, 0, keepalive=replica_mem)
    assert key3.prove(wb, r, s) == proof


def test_packed_key_file_roundtrip(tmp_path, small_case):
    """zkr_key_save / zkr_key_load_file: the reloaded key proves bit-identically; a truncated, foreign or
    header-damaged file is refused."""
    import zkr_hip
    c = small_case
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    path = str(tmp_path / "tx.zkrkey")
    key.save(path)
    key2 = zkr_hip.ProvingKey.load_file(path)
    assert key2.info() == key.info() and key2.windows() == key.windows()
    assert key2.prove(c["wb"], c["r"], c["s"]) == key.prove(c["wb"], c["r"], c["s"]) == coracle.prove(c["pkb"], c["wb"], c["r"], c["s"])
    blob = open(path, "rb").read()
    bad = str(tmp_path / "bad.zkrkey")
    open(bad, "wb").write(blob[:-7])
    with pytest.raises(zkr_hip.ZkrError):
        zkr_hip.ProvingKey.load_file(bad)
    open(bad, "wb").write(b"\0" * 4096)
    with pytest.raises(zkr_hip.ZkrError):
        zkr_hip.ProvingKey.load_file(bad)
    # a header whose sizes or offsets were altered (right magic, right length) is refused before any kernel reads through it:
    # off_tw at byte 64, npts[0] at byte 40, nnzA at byte 32 of the arena header (csrc/zkr_internal.hpp ArenaHeader)
    for at, width, delta in ((64, 8, 4096), (40, 4, 1), (32, 4, -1), (16, 4, 7)):
        v = int.from_bytes(blob[at:at + width], "little") + delta
        open(bad, "wb").write(blob[:at] + v.to_bytes(width, "little") + blob[at + width:])
        with pytest.raises(zkr_hip.ZkrError):
            zkr_hip.ProvingKey.load_file(bad)


def test_dense_random_shape_matches_oracle_generator():
    """BASELINE configs[4] shape (dense random R1CS: no infinity points in any query): product-side generator +
    device setup == oracle generator + setup byte for byte, proof == oracle proof == closed form."""
    import zkr_hip
    log_m, p = 8, 5
    zkr_hip.synth_set_shape(1)
    try:
        pkb, wb = zkr_hip.synth_websnark(log_m, p, 0x5A4B0005, 0x5A4B00FF)
        key2, wb2, _ = zkr_hip.ProvingKey.synth(log_m, p, 0x5A4B0005, 0x5A4B00FF)
    finally:
        zkr_hip.synth_set_shape(0)
    circ = g.synth_circuit(1 << log_m, p, 0x5A4B0005, shape=1)
    assert g.check_r1cs(circ) and circ["nVars"] == 1 << log_m
    assert g.binarify_witness(circ["witness"]) == wb == wb2
    tox = g.toxic_from_seed(0x5A4B00FF)
    pk, _ = g.setup(circ, tox)
    assert g.binarify_proving_key(g.to_json_key(pk)) == pkb
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    info = key.info()
    # far fewer infinity points than the rollup shape (a third of B there): only the newest signals are still unused
    assert info["ptsB1"] == info["ptsB2"] >= 0.75 * circ["nVars"] and info["ptsA"] >= 0.75 * circ["nVars"]
    rng = g.SplitMix64(55)
    r, s = rng.fr(), rng.fr()
    proof = key.prove(wb, r, s)
    assert proof == coracle.prove(pkb, wb, r, s) == g.proof_bytes(g.proof_from_toxic(circ, tox, circ["witness"], r, s))
    assert key2.prove(wb, r, s) == proof


def test_reference_caller_pattern_new_object_per_proof_uses_the_process_cache(small_case):
    """operator/src/snarks/common.ts:23-29 calls `buildBn128()` and `binarifyProvingKey()` for every proof: with the
    process-level cache (facade.cached_key) only the first call loads the key; three keys rotate through two slots."""
    import zkr_hip
    c = small_case
    zkr_hip.clear_key_cache()
    before = dict(zkr_hip.key_cache_stats)
    expect = zkr_hip.proof_json_from_bytes(coracle.prove(c["pkb"], c["wb"], c["r"], c["s"]))
    for _ in range(3):
        bn = zkr_hip.build_bn128()                                            # a fresh object per proof
        assert bn.groth16GenProof(c["wb"], bytes(c["pkb"]), c["r"], c["s"]) == expect
    assert zkr_hip.key_cache_stats["loads"] - before["loads"] == 1 and zkr_hip.key_cache_stats["hits"] - before["hits"] == 2
    def other(k):                                                             # swap two hExps points: another (valid) key
        b = bytearray(c["pkb"])
        b[-64:], b[-64 * (k + 1):-64 * k] = b[-64 * (k + 1):-64 * k], b[-64:]
        return bytes(b)
    zkr_hip.groth16_gen_proof(c["wb"], other(1))
    zkr_hip.groth16_gen_proof(c["wb"], other(2))                              # evicts the first key
    zkr_hip.groth16_gen_proof(c["wb"], other(1))
    assert zkr_hip.key_cache_stats["loads"] - before["loads"] == 3
    assert zkr_hip.groth16_gen_proof(c["wb"], c["pkb"], r=c["r"], s=c["s"]) == expect
    assert zkr_hip.key_cache_stats["loads"] - before["loads"] == 4
    zkr_hip.clear_key_cache()


def test_proof_facade_like_reference_tests(small_case):
    """createProofGenerator flow of common.ts:10-53 on the product only (HIP prover + native isValid), asserted the way
    contracts/__tests__/withdrawverifier.test.ts:24-65 does: valid proof, inputs in order, wrong key -> 'Invalid proof generated'."""
    import zkr_hip
    c = small_case
    gen = zkr_hip.create_proof_generator(c["pkb"], c["vk"], n_public=7)
    out = gen(c["w"], c["r"], c["s"])
    assert out["proof"] == g.proof_to_json(g.proof_from_toxic(c["circ"], c["tox"], c["w"], c["r"], c["s"]))
    sol = out["solidityProof"]
    assert sol["inputs"] == [str(x) for x in c["w"][1:8]]                                  # withdrawverifier.test.ts:35-37
    assert sol["b"][0] == [out["proof"]["pi_b"][0][1], out["proof"]["pi_b"][0][0]]          # common.ts:45-47 (im, re)
    assert zkr_hip.is_valid(c["vk"], out["proof"], sol["inputs"])
    tampered = list(sol["inputs"])
    tampered[0] = str((int(tampered[0]) + 1) % g.R)
    assert not zkr_hip.is_valid(c["vk"], out["proof"], tampered)                            # withdrawverifier.test.ts:56-65
    # a verifying key of another setup must make the facade throw (common.ts:36-38)
    _, vk2 = g.setup(c["circ"], g.toxic_from_seed(0x1234))
    with pytest.raises(zkr_hip.ZkrError, match="Invalid proof generated"):
        zkr_hip.create_proof_generator(c["pkb"], vk2, n_public=7)(c["w"], c["r"], c["s"])


@pytest.mark.parametrize("kind", ["only_one", "all_max", "booleans", "small64", "zeros_mixed"])
def test_degenerate_witnesses_match_oracle(small_case, kind):
    """Witness shapes that stress the digit sort and the bucket paths through the whole proof (they do not satisfy the
    circuit; prover and oracle must still compute the same group elements, as the reference algorithm would):
    only w_0 = 1, every signal r-1, 0/1 signals (one oversized bucket), 64-bit values (most windows empty), and a
    zero-heavy mix."""
    import zkr_hip
    c = small_case
    n = len(c["w"])
    rnd = random.Random(sum(map(ord, kind)))
    w = {
        "only_one": [1] + [0] * (n - 1),
        "all_max": [1] + [R - 1] * (n - 1),
        "booleans": [1] + [rnd.randrange(2) for _ in range(n - 1)],
        "small64": [1] + [rnd.randrange(1 << 64) for _ in range(n - 1)],
        "zeros_mixed": [1] + [0 if i % 3 else rnd.randrange(R) for i in range(n - 1)],
    }[kind]
    wb = g.binarify_witness(w)
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    assert key.prove(wb, c["r"], c["s"]) == coracle.prove(c["pkb"], wb, c["r"], c["s"])
    assert key.calc_h(wb) == b"".join(_le(x) for x in g.calc_h_websnark(c["pk"], w))


def test_setup_of_an_r1cs_on_the_gpu_matches_oracle_setup(small_case):
    """zkr_setup_r1cs (`snarkjs setup --protocol groth`, prover/package.json:34,37): same toxic waste ->
    the verifying key equals the oracle's setup and proofs equal the closed form; fresh CSPRNG toxic waste -> proofs
    verify under the returned key and differ from the seeded setup's."""
    import zkr_hip
    c = small_case
    circ, tox = c["circ"], c["tox"]
    cdef = dict(nVars=circ["nVars"], nPubInputs=5, nOutputs=2,
                constraints=[[{str(s): str(cf) for s, cf in lc} for lc in row] for row in circ["rows"]])
    r1cs = zkr_hip.binarify_r1cs(cdef)
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=[tox[k] for k in ("t", "alfa", "beta", "gamma", "delta")])
    assert vk_bin == zkr_hip.binarify_verifying_key(c["vk"])
    assert key.info()["domainSize"] == 128 and key.info()["nVars"] == circ["nVars"]
    proof = key.prove(c["wb"], c["r"], c["s"])
    assert proof == g.proof_bytes(g.proof_from_toxic(circ, tox, c["w"], c["r"], c["s"]))
    pub = c["w"][1:8]
    assert zkr_hip.verify(vk_bin, proof, pub)
    vkj = zkr_hip.verifying_key_from_bytes(vk_bin)
    assert zkr_hip.is_valid(vkj, zkr_hip.proof_json_from_bytes(proof), pub) and vkj["nPublic"] == 7
    # a circuit that does not fill its domain: nConstraints + nPublic + 1 = 61 -> domainSize 64
    small = dict(nVars=circ["nVars"], nPublic=7, constraints=[[list(lc) for lc in row] for row in circ["rows"][:53]])
    key2, vk2 = zkr_hip.ProvingKey.setup_r1cs(zkr_hip.binarify_r1cs(small))      # CSPRNG toxic waste
    assert key2.info()["domainSize"] == 64
    p2 = key2.prove(c["wb"], c["r"], c["s"])   # the witness satisfies the first 53 constraints as well
    assert zkr_hip.verify(vk2, p2, pub) and p2 != proof
    bad = list(pub)
    bad[0] = (bad[0] + 1) % R
    assert not zkr_hip.verify(vk2, p2, bad)
    with pytest.raises(zkr_hip.ZkrError):
        zkr_hip.ProvingKey.setup_r1cs(r1cs[:-3])


@pytest.mark.parametrize("name", ["synth_m5.json", "synth_m7.json", "synth_m10.json"])
def test_hip_path_reproduces_committed_golden_fixtures(name):
    """The committed fixtures (tests/golden/, written by make_golden.py from the oracle) through the product only:
    generator + device setup give the fixture's key and witness bytes, calcH its h, the prover its proof bytes, the
    facade its solidityProof."""
    import hashlib
    import json
    import os
    import zkr_hip
    fx = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)))
    pkb, wb = zkr_hip.synth_websnark(int(fx["log_m"]), int(fx["n_public"]), int(fx["circuit_seed"]), int(fx["toxic_seed"]))
    sha = lambda b: hashlib.sha256(b).hexdigest()
    assert (sha(pkb), len(pkb), sha(wb)) == (fx["pk_bin_sha256"], int(fx["pk_bin_len"]), fx["witness_bin_sha256"])
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    h = key.calc_h(wb)
    assert sha(h) == fx["h_sha256"]
    assert [str(int.from_bytes(h[32 * i:32 * i + 32], "little")) for i in range(4)] == list(fx["h_first4"])
    proof = key.prove(wb, int(fx["r"]), int(fx["s"]))
    assert proof.hex() == fx["proof_bytes_hex"]
    pj = zkr_hip.proof_json_from_bytes(proof)
    assert pj == fx["proof"]
    pub = [int.from_bytes(wb[32 * i:32 * i + 32], "little") for i in range(1, int(fx["n_public"]) + 1)]
    assert zkr_hip.solidity_proof(pj, pub) == fx["solidity_proof"]


def test_prove_batch_from_host_buffers_equals_single_proofs(small_case):
    """zkr_prove_batch (host witnesses, uploads and proofs pipelined over the key's workspaces) == zkr_prove one by one ==
    the oracle; a witness of the wrong length is refused before anything is enqueued."""
    import zkr_hip
    c = small_case
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    wits, rs, ss = [], [], []
    for i in range(5):
        wb = c["wb"] if i % 2 == 0 else zkr_hip.synth_witness(7, 7, 0x5A4B0001, 900 + i)
        wits.append(wb)
        rs.append(1000 + i)
        ss.append(2000 + i)
    proofs = key.prove_batch(wits, rs, ss)
    assert len(proofs) == 5
    for i in range(5):
        assert proofs[i] == key.prove(wits[i], rs[i], ss[i]) == coracle.prove(c["pkb"], wits[i], rs[i], ss[i])
    assert key.prove_batch([]) == []
    with pytest.raises(zkr_hip.ZkrError) as e:
        key.prove_batch([wits[0][:-32]])
    assert e.value.code == -3
    assert key.prove(wits[1], 5, 6) == coracle.prove(c["pkb"], wits[1], 5, 6)      # the key is still usable


@pytest.mark.parametrize("count", [1, 4])
def test_c_and_h_in_chains_of_their_own(count):
    """A circuit with far fewer signals than constraints (100 under a domain of 2^8: tests/layout_cases.py): C's window follows the
    signals, H's the domain, so H cannot land on C's bucket set and each is reduced by a chain of its own, H's last (csrc/msm_plan.hpp
    proof_layout).  One proof alone and a fused batch of four, unsatisfied witnesses among them, against the oracle."""
    import zkr_hip
    from layout_cases import few_signals_many_constraints
    c = few_signals_many_constraints()
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    info, win = key.info(), key.windows()
    assert (info["nVars"], info["domainSize"]) == (100, 256) and info["ptsC"] > 0 and info["ptsH"] > 0
    assert win["C"][0] == win["A"][0] == 7 and win["H"][0] == 8 and key.fuse() >= 4
    rnd = random.Random(count)
    wits = [c["wb"]] + [g.binarify_witness([1] + [rnd.randrange(R) for _ in range(99)]) for _ in range(count - 1)]
    rs, ss = [rnd.randrange(R) for _ in wits], [rnd.randrange(R) for _ in wits]
    want = [coracle.prove(c["pkb"], wb, r, s) for wb, r, s in zip(wits, rs, ss)]
    assert want[0] == g.proof_bytes(g.proof_from_toxic(c["circ"], g.toxic_from_seed(0x5A4B00FF), c["w"], rs[0], ss[0]))
    got = key.prove_batch(wits, rs, ss) if count > 1 else [key.prove(wits[0], rs[0], ss[0])]
    assert got == want


_SORT_KNOB_CHILD = r"""
import random, sys
sys.path[:0] = %r
import coracle, zkr_hip
from bn254 import Q, R, G1_GEN, g1_add, g1_mul
MONT = 1 << 256
le = lambda v: int(v).to_bytes(32, "little")
rnd = random.Random(77)
pts, P = [], G1_GEN
for i in range(300):
    pts.append(None if i %% 7 == 3 else P)
    P = g1_add(P, G1_GEN) if i %% 5 else g1_mul(P, 3)
for n in (1000, 20000):
    sc = [rnd.randrange(R) for _ in range(n)]
    for i in range(0, n, 11):
        sc[i] = rnd.choice([0, 1, 1, 2, R - 1, (1 << 64) - 1, 1 << 253])
    pb = b"".join(le(0) + le(MONT %% Q) if pts[i %% 300] is None else le(pts[i %% 300][0] * MONT %% Q) + le(pts[i %% 300][1] * MONT %% Q) for i in range(n))
    sb = b"".join(le(x) for x in sc)
    assert zkr_hip.msm_g1(pb, sb) == coracle.msm_g1(pb, sb), n
print("sort knobs ok")
"""


@pytest.mark.parametrize("knobs", [
    {"ZKR_MSM_C": "8"},    # narrow windows: K = 32 levels, 128 buckets (the unstaged record kernels, one bucket range)
    {"ZKR_MSM_C": "13"},   # 4096 buckets: two bucket ranges, lanes shared per bucket in the accumulation
], ids=lambda k: ",".join("%s=%s" % kv for kv in k.items()))
def test_window_size_knob_changes_no_result(knobs):
    """ZKR_MSM_C (window bits; the one plan knob the library keeps) is read when the library plans a key, so each setting runs in
    its own process: the sort / accumulation / reduction geometry that follows from it gives the oracle's MSM results."""
    import os, subprocess, sys
    env = dict(os.environ, **knobs)
    out = subprocess.run([sys.executable, "-c", _SORT_KNOB_CHILD % (sys.path,)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "sort knobs ok" in out.stdout, out.stderr[-2000:]


_KNOB_SCRIPT = r"""
import os, sys
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "simple-zk-rollups_amd", "python")); sys.path.insert(0, os.path.join(root, "oracle"))
import groth16 as g, zkr_hip
ok = True
for log_m, count in ((9, 3), (13, 9), (17, 2)):
    key, wb, aux = zkr_hip.ProvingKey.synth(log_m, 73 if log_m >= 10 else 5, 0x5A4B0001, 0x5A4B00FF)
    p = 73 if log_m >= 10 else 5
    rs, ss = [11 + i for i in range(count)], [29 + i for i in range(count)]
    got = key.prove_batch([wb] * count, rs, ss)
    for i in range(count):
        ok = ok and got[i] == g.proof_bytes(g.proof_from_aux(aux, wb, p, rs[i], ss[i])[0])
    ok = ok and key.prove(wb, 5, 6) == g.proof_bytes(g.proof_from_aux(aux, wb, p, 5, 6)[0])
print("PARITY", ok)
"""


@pytest.mark.parametrize("env", [{"ZKR_SERIAL": "1"}, {"ZKR_MSM_C": "11"}])
def test_schedule_and_window_knobs_give_the_same_proofs(tmp_path, env):
    """The two proving-path knobs the library keeps are read once per process: the serial schedule (one stream, the profiling
    aid: every launch in order on one stream; the joint A / B1 chain stays) and another window size each run in their own process and must reproduce
    the closed form -- single proofs and fused batches, 2^9 to 2^17."""
    import subprocess
    import sys
    script = tmp_path / "knobs.py"
    script.write_text(_KNOB_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and "PARITY True" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])
