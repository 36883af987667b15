"""The powers-of-tau transcript on the MI355X: the group arithmetic under it (zkr_points_scale_each, zkr_group_ntt), contributions
and their records (zkr_ptau_contribute), the verification (zkr_ptau_verify) and the setup of a key from a transcript
(zkr_setup_r1cs_ptau).

Everything is compared EXACTLY, as bytes or points.  The expected values come from the oracle (oracle/bn254.py,
oracle/groth16.py: fixed-base tables of the generators, the scalar NTT, lagrange_at, proof_from_toxic) and from the existing
zkr_setup_r1cs with injected toxic values, never from the code under test: a point of a test is log * G for a log the test knows,
and the library must return (what the oracle makes of the logs) * G.

The transform has ONE code path for every size (bit reversal, then a launch per stage over global memory), so there is no switch
to straddle; the sizes cover one butterfly (logn 1), stages inside one wavefront, and several workgroups (logn 10: 512
butterflies in two workgroups of 256).  The scaling kernel gives a thread n / 2^18 points, at least one and at most eight: one
point up to 2^19 - 1 points (every transcript and transform of this file, the power-17 one included), two from 2^19.  The case
n = 2^19 + 3 is there for that path: two points per thread with their shared inversion, and a ragged tail in which some
threads hold one.

Safety: the tampered transcripts are made on the host from valid ones and keep the layout; each is ONE call, run once.  What a
kernel reads from them is bounded by the header, which is checked first, and every coordinate and curve equation is checked on
the device before any group arithmetic touches the data."""
import pytest

import groth16 as g
from bn254 import Q, R, G1_GEN, G2_GEN

pytestmark = pytest.mark.gpu
MONT = 1 << 256

TAU1, ALFA1, BETA1 = 0x1A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F7081, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978, 0x123456789ABCDEF0FEDCBA9876543210123456789ABCDEF
TAU2, ALFA2, BETA2 = 0x2468ACE013579BDF02468ACE13579BDF2468ACE013579BDF0246, 0x1F2E3D4C5B6A79880112233445566778899AABBCCDDEEFF, 0x0CAFEBABEDEADBEEF0123456789ABCDEFFEDCBA9876543210CAFE


def _le(v):
    return int(v).to_bytes(32, "little")


def _mont1(P):
    return bytes(64) if P is None else _le(P[0] * MONT % Q) + _le(P[1] * MONT % Q)


def _mont2(P):
    return bytes(128) if P is None else b"".join(_le(c * MONT % Q) for c in (P[0][0], P[0][1], P[1][0], P[1][1]))


def _std1(P):
    return _le(P[0]) + _le(P[1])


def _std2(P):
    return b"".join(_le(c) for c in (P[0][0], P[0][1], P[1][0], P[1][1]))


class _Gen:
    """k * generator by the oracle's fixed-base tables, remembered per scalar (None = infinity)."""

    def __init__(self):
        self.fb = g._fb()
        self.seen = ({}, {})

    def mul(self, k, g2=False):
        k %= R
        c = self.seen[1 if g2 else 0]
        if k not in c:
            c[k] = None if k == 0 else self.fb[1 if g2 else 0].mul(k)
        return c[k]

    def mont(self, logs, g2=False):
        return b"".join((_mont2 if g2 else _mont1)(self.mul(k, g2)) for k in logs)


@pytest.fixture(scope="module")
def gen():
    return _Gen()


# ---------------------------------------------------------------- points_scale_each
SCALARS = [0, 1, 2, R - 1, R - 2, (1 << 128) - 159, 3, 0x183227397098D014DC2822DB40C0AC2ECBC0B548B438E5469E10460B6C3E7EA3 % R,
           0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE1234567890ABCDEF % R, R >> 1, (1 << 253) + 12345, 0x5EED]
LOGS = [1, 0, 2, R - 1, 0x1D0C5EED0123456789ABCDEF02468ACE13579BDF, 7, (R + 1) // 2, 0xDEADBEEF]   # 0: an infinity entry


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_points_scale_each_matches_the_oracle(gen, n, g2):
    import zkr_hip
    if n == 1:
        logs, sc = [LOGS[4]], [SCALARS[7]]
    else:   # every (log, scalar) pair of the two pools, over and over
        logs = [LOGS[i % 8] for i in range(n)]
        sc = [SCALARS[(i // 8) % 12] for i in range(n)]
        assert len({(a, b) for a, b in zip(logs, sc)}) == 96
    out = zkr_hip.points_scale_each(gen.mont(logs, g2), b"".join(_le(s) for s in sc), g2=g2)
    want = gen.mont([a * b % R for a, b in zip(logs, sc)], g2)
    pb = 128 if g2 else 64
    bad = [i for i in range(n) if out[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
    assert bad == []


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_points_scale_each_with_several_points_per_thread_and_a_ragged_tail(gen, g2):
    """n = 2^19 + 3: two points per thread (the prefix products of the shared inversion) in 1 025 workgroups, whose last 509
    threads hold one point only.  The 96 (log, scalar) pairs of the pools repeat, so the oracle multiplies nothing new."""
    import zkr_hip
    n, pb = (1 << 19) + 3, 128 if g2 else 64
    pairs = [(LOGS[i % 8], SCALARS[(i // 8) % 12]) for i in range(96)]
    reps, rest = divmod(n, 96)
    tile = lambda block: block * reps + block[:rest * (len(block) // 96)]
    out = zkr_hip.points_scale_each(tile(gen.mont([a for a, _ in pairs], g2)), tile(b"".join(_le(s) for _, s in pairs)), g2=g2)
    want = tile(gen.mont([a * b % R for a, b in pairs], g2))
    assert len(out) == len(want) == n * pb
    if out != want:
        bad = [i for i in range(n) if out[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
        assert (len(bad), bad[:8]) == (0, [])


def test_points_scale_each_refuses_a_scalar_not_below_r(gen):
    import zkr_hip
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.points_scale_each(gen.mont([1, 2]), _le(5) + _le(R))
    assert e.value.code == -5 and "scalar 1" in str(e.value)


# ---------------------------------------------------------------- group_ntt
NTT_SIZES = [(1, False), (2, False), (3, False), (8, False), (10, False), (1, True), (3, True), (6, True)]


def _rand_logs(n, seed):
    rng = g.SplitMix64(seed)
    return [rng.fr() for _ in range(n)]


@pytest.mark.parametrize("logn,g2", NTT_SIZES, ids=["%s_%d" % ("g2" if b else "g1", l) for l, b in NTT_SIZES])
def test_group_ntt_is_the_scalar_ntt_in_the_exponent(gen, logn, g2):
    import zkr_hip
    n = 1 << logn
    logs = _rand_logs(n, 0xA11CE + logn)
    if n >= 4:
        logs[1] = 0          # infinities in the input
        logs[n - 1] = 0
    pts = gen.mont(logs, g2)
    fwd = zkr_hip.group_ntt(pts, g2=g2)
    assert fwd == gen.mont(g.ntt(logs), g2)
    inv = zkr_hip.group_ntt(pts, inverse=True, g2=g2)
    assert inv == gen.mont(g.ntt(logs, invert=True), g2)
    assert zkr_hip.group_ntt(fwd, inverse=True, g2=g2) == pts


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_group_ntt_of_equal_points_drives_the_butterflies_through_doubling_and_cancellation(gen, g2):
    import zkr_hip
    logn, k = 4, 0xC0FFEE
    n = 1 << logn
    out = zkr_hip.group_ntt(gen.mont([k] * n, g2), g2=g2)
    assert out == gen.mont([n * k] + [0] * (n - 1), g2)       # (n P, O, ..., O): P + P and P - P in every stage
    assert zkr_hip.group_ntt(out, inverse=True, g2=g2) == gen.mont([k] * n, g2)


@pytest.mark.parametrize("logn,g2", [(5, False), (3, True)], ids=["g1_5", "g2_3"])
def test_inverse_group_ntt_of_the_powers_of_tau_gives_the_lagrange_basis_points(gen, logn, g2):
    import zkr_hip
    m, tau = 1 << logn, TAU1 * TAU2 % R
    out = zkr_hip.group_ntt(gen.mont([pow(tau, i, R) for i in range(m)], g2), inverse=True, g2=g2)
    assert out == gen.mont(g.lagrange_at(m, tau), g2)


# ---------------------------------------------------------------- the transcript
def _closed_form(gen, K, tau, alfa, beta):
    M = 1 << K
    tp = [pow(tau, i, R) for i in range(2 * M)]
    body = (b"".join(_std1(gen.mul(t)) for t in tp) + b"".join(_std2(gen.mul(t, True)) for t in tp[:M]) +
            b"".join(_std1(gen.mul(alfa * t)) for t in tp[:M]) + b"".join(_std1(gen.mul(beta * t)) for t in tp[:M]) + _std2(gen.mul(beta, True)))
    total = 160 + 384 * M
    return b"ZKRPTAU1" + K.to_bytes(4, "little") + bytes(4) + total.to_bytes(8, "little") + bytes(8) + body


@pytest.fixture(scope="module")
def chains(gen):
    """K -> (transcript after one contribution, after two, [record 1, record 2])."""
    import zkr_hip
    out = {}
    for K in (3, 5):
        p1, r1 = zkr_hip.ptau_contribute(zkr_hip.ptau_new(K), (TAU1, ALFA1, BETA1))
        p2, r2 = zkr_hip.ptau_contribute(p1, (TAU2, ALFA2, BETA2))
        out[K] = (p1, p2, [r1, r2])
    return out


@pytest.mark.parametrize("K", [3, 5])
def test_two_chained_contributions_give_the_closed_form_of_the_product_secrets(gen, chains, K):
    import zkr_hip
    p1, p2, recs = chains[K]
    want1 = _closed_form(gen, K, TAU1, ALFA1, BETA1)
    assert len(p1) == len(want1) == 160 + 384 * (1 << K)
    assert p1 == want1
    assert p2 == _closed_form(gen, K, TAU1 * TAU2 % R, ALFA1 * ALFA2 % R, BETA1 * BETA2 % R)
    assert len(recs[0]) == len(recs[1]) == zkr_hip.PTAU_RECORD_BYTES
    assert zkr_hip.ptau_record_check(recs) is True
    assert zkr_hip.ptau_record_check(recs[:1]) is True
    assert zkr_hip.ptau_record_check(recs[::-1]) is False
    # the record is about THESE transcripts
    M = 1 << K
    o_tau1, o_tau2, o_alfa, o_beta, o_beta2 = 32 + 64, 32 + 128 * M + 128, 32 + 256 * M, 32 + 320 * M, 32 + 384 * M
    r2 = recs[1]
    assert r2[0:64] == p1[o_tau1:o_tau1 + 64] and r2[64:128] == p2[o_tau1:o_tau1 + 64]
    assert r2[128:192] == p1[o_alfa:o_alfa + 64] and r2[192:256] == p2[o_alfa:o_alfa + 64]
    assert r2[256:320] == p1[o_beta:o_beta + 64] and r2[320:384] == p2[o_beta:o_beta + 64]
    assert r2[384:512] == p2[o_tau2:o_tau2 + 128] and r2[512:640] == p2[o_beta2:o_beta2 + 128]


def test_a_contribution_with_secrets_drawn_inside_the_library_has_a_valid_record_and_differs_each_time(chains):
    import zkr_hip
    p1, _, recs = chains[3]
    a, ra = zkr_hip.ptau_contribute(p1)
    b, rb = zkr_hip.ptau_contribute(p1)
    assert zkr_hip.ptau_record_check([recs[0], ra]) is True and zkr_hip.ptau_record_check([recs[0], rb]) is True
    assert a != b and a != p1 and ra[64:128] != rb[64:128]


def test_contribute_refuses_bad_input_before_any_group_arithmetic(chains):
    import zkr_hip
    p1 = chains[3][0]
    y = int.from_bytes(p1[32 + 64 * 5 + 32:32 + 64 * 6], "little")
    cases = {
        "truncated": p1[:-1],
        "magic": b"ZKRPTAU0" + p1[8:],
        "off the curve": p1[:32 + 64 * 5 + 32] + _le((y + 1) % Q) + p1[32 + 64 * 6:],
        "coordinate not below q": p1[:32 + 64 * 5 + 32] + _le(y + Q) + p1[32 + 64 * 6:],
        "infinity": p1[:32 + 64 * 5] + bytes(64) + p1[32 + 64 * 6:],
    }
    for what, bad in cases.items():
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.ptau_contribute(bad, (TAU2, ALFA2, BETA2))
        assert e.value.code == -5, what
    for sec in [(1, ALFA1, BETA1), (TAU1, 0, BETA1), (TAU1, ALFA1, R)]:
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.ptau_contribute(p1, sec)
        assert e.value.code == -5 and "1 < s < r" in str(e.value)


# ---------------------------------------------------------------- ptau_verify
V_TAU1, V_TAU2, V_ALFA1, V_BETA1, V_BETA2 = range(5)


def _off(K):
    M = 1 << K
    return {V_TAU1: 32, V_TAU2: 32 + 128 * M, V_ALFA1: 32 + 256 * M, V_BETA1: 32 + 320 * M, V_BETA2: 32 + 384 * M}


def _put(t, off, piece):
    return t[:off] + piece + t[off + len(piece):]


@pytest.mark.parametrize("K", [3, 5])
def test_verify_accepts_the_chain_and_its_records(chains, K):
    import zkr_hip
    p1, p2, recs = chains[K]
    assert zkr_hip.ptau_verify(p2, recs)[:2] == (True, 0)
    assert zkr_hip.ptau_verify(p1, recs[:1])[:2] == (True, 0)


def test_the_smallest_transcript_contributes_and_verifies():
    """Power 1 (M = 2): the sums of step 5 have three points and one."""
    import zkr_hip
    start = zkr_hip.ptau_new(1)
    assert zkr_hip.ptau_verify(start)[:2] == (True, 0)
    t, rec = zkr_hip.ptau_contribute(start, (TAU1, ALFA1, BETA1))
    assert zkr_hip.ptau_verify(t, [rec])[:2] == (True, 0)
    assert zkr_hip.ptau_verify(t)[:2] == (False, 6)


def test_verify_accepts_the_start_without_records_and_a_contribution_with_drawn_secrets(chains):
    import zkr_hip
    assert zkr_hip.ptau_verify(zkr_hip.ptau_new(3))[:2] == (True, 0)
    p1, _, recs = chains[3]
    a, ra = zkr_hip.ptau_contribute(p1)
    assert zkr_hip.ptau_verify(a, [recs[0], ra])[:2] == (True, 0)


def _tampered(gen, chains):
    """name -> (transcript, records, step, vector): copies of the valid K = 3 transcript with ONE thing wrong, made on the host."""
    from test_contribution_cpu import twist_point_outside_g2
    K, M = 3, 8
    _, p2, recs = chains[K]
    o = _off(K)
    tau, alfa, beta = TAU1 * TAU2 % R, ALFA1 * ALFA2 % R, BETA1 * BETA2 % R
    e3, e5 = p2[o[V_TAU1] + 64 * 3:o[V_TAU1] + 64 * 4], p2[o[V_TAU1] + 64 * 5:o[V_TAU1] + 64 * 6]
    y = int.from_bytes(p2[o[V_BETA1] + 64 * 2 + 32:o[V_BETA1] + 64 * 3], "little")
    return {
        "two entries of tauG1 swapped": (_put(_put(p2, o[V_TAU1] + 64 * 3, e5), o[V_TAU1] + 64 * 5, e3), recs, 5, V_TAU1),
        "an alfaTauG1 entry for another alfa": (_put(p2, o[V_ALFA1] + 64 * 4, _std1(gen.mul((alfa + 1) * pow(tau, 4, R)))), recs, 5, V_ALFA1),
        "a tauG2 entry replaced by another point of G2": (_put(p2, o[V_TAU2] + 128 * 3, _std2(gen.mul(12345, True))), recs, 5, V_TAU2),
        "a tauG2 entry on the twist outside G2": (_put(p2, o[V_TAU2] + 128 * 6, _std2(twist_point_outside_g2())), recs, 3, V_TAU2),
        "betaG2 for another beta": (_put(p2, o[V_BETA2], _std2(gen.mul(beta + 1, True))), recs, 5, V_BETA2),
        "a coordinate moved off the curve": (_put(p2, o[V_BETA1] + 64 * 2 + 32, _le((y + 1) % Q)), recs, 2, V_BETA1),
        "an infinity entry": (_put(p2, o[V_TAU1] + 64 * 9, bytes(64)), recs, 2, V_TAU1),
        "a coordinate not below q": (_put(p2, o[V_ALFA1] + 64 * 5, _le(int.from_bytes(p2[o[V_ALFA1] + 64 * 5:o[V_ALFA1] + 64 * 5 + 32], "little") + Q)), recs, 2, V_ALFA1),
        "tauG1 does not start at the generator": (_put(p2, o[V_TAU1], _std1(gen.mul(2))), recs, 4, V_TAU1),
        "the records of another transcript": (p2, recs[:1], 6, None),
        "no records for a contributed transcript": (p2, [], 6, None),
    }


@pytest.mark.parametrize("what", ["two entries of tauG1 swapped", "an alfaTauG1 entry for another alfa", "a tauG2 entry replaced by another point of G2",
                                  "a tauG2 entry on the twist outside G2", "betaG2 for another beta", "a coordinate moved off the curve", "an infinity entry", "a coordinate not below q",
                                  "tauG1 does not start at the generator", "the records of another transcript", "no records for a contributed transcript"])
def test_verify_refuses_and_names_the_step(gen, chains, what):
    import zkr_hip
    t, recs, step, vector = _tampered(gen, chains)[what]
    ok, got_step, got_vector = zkr_hip.ptau_verify(t, recs)          # one call, run once
    assert (ok, got_step) == (False, step), zkr_hip.lib().zkr_last_error().decode()
    if vector is not None:
        assert got_vector == vector
    assert ("step %d" % step) in zkr_hip.lib().zkr_last_error().decode()


def test_verify_answers_a_truncated_buffer_and_a_wrong_magic_with_an_error_status(chains):
    import zkr_hip
    p2 = chains[3][1]
    for bad in (p2[:-64], b"ZKRPTAU2" + p2[8:]):
        with pytest.raises(zkr_hip.ZkrError) as e:
            zkr_hip.ptau_verify(bad, chains[3][2])
        assert e.value.code == -5 and "step 1" in str(e.value)


# ---------------------------------------------------------------- setup_r1cs_ptau
D = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE
TAU, ALFA, BETA = TAU1 * TAU2 % R, ALFA1 * ALFA2 % R, BETA1 * BETA2 % R


def _transcript(K, two=True):
    import zkr_hip
    t, _ = zkr_hip.ptau_contribute(zkr_hip.ptau_new(K), (TAU1, ALFA1, BETA1))
    if two:
        t, _ = zkr_hip.ptau_contribute(t, (TAU2, ALFA2, BETA2))
    return t


def _file(key, path):
    key.save(str(path))
    return open(path, "rb").read()


def _same_key_as_the_toxic_setup(r1cs, ptau, toxic, tmp_path):
    import zkr_hip
    kp, vkp = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, ptau)
    kt, vkt = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=toxic)
    try:
        assert vkp == vkt
        fp, ft = _file(kp, tmp_path / "ptau.zkr"), _file(kt, tmp_path / "toxic.zkr")
        assert len(fp) == len(ft)
        assert fp == ft
        assert kp.check(level=1)["bad"] == 0
    finally:
        kp.close()
        kt.close()


@pytest.mark.parametrize("K", [7, 9], ids=["exact_power", "prefix_of_a_larger_transcript"])
def test_setup_from_a_transcript_is_the_toxic_setup_byte_for_byte_small(K, tmp_path):
    from test_gpu_contribution import _small
    r1cs = _small()[0]
    _same_key_as_the_toxic_setup(r1cs, _transcript(K), [TAU, ALFA, BETA, 1, 1], tmp_path)


def test_setup_from_a_transcript_is_the_toxic_setup_byte_for_byte_tx_circuit(tmp_path):
    """The one real-size case: BatchProcessTx(2, 6), domain 2^17 -- long columns (signal 0) and the transforms across every stage."""
    from test_gpu_contribution import _tx
    r1cs = _tx()[0]
    _same_key_as_the_toxic_setup(r1cs, _transcript(17, two=False), [TAU1, ALFA1, BETA1, 1, 1], tmp_path)


def test_the_flow_ends_in_an_accepted_proof():
    import zkr_hip
    from test_gpu_contribution import _small
    r1cs, wb, pub, _ = _small()
    circ = g.synth_circuit(128, 7, 0x5A4B0001)
    k0, vk0 = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, _transcript(7))
    k1, rec = k0.contribute(D)
    try:
        rng = g.SplitMix64(20261017)
        r, s = rng.fr(), rng.fr()
        proof = k1.prove(wb, r, s)
        assert proof == g.proof_bytes(g.proof_from_toxic(circ, dict(t=TAU, alfa=ALFA, beta=BETA, gamma=1, delta=D), circ["witness"], r, s))
        vk1 = zkr_hip.vk_contribute(vk0, rec)
        assert zkr_hip.verify(vk1, proof, pub) is True
        assert zkr_hip.verify(vk1, proof, [pub[0] + 1] + list(pub[1:])) is False
        assert zkr_hip.verify(vk0, proof, pub) is False      # delta = 1 is not this proof's key
    finally:
        k1.close()
        k0.close()


def test_setup_refuses_a_transcript_that_is_too_small_or_does_not_verify(chains):
    import zkr_hip
    from test_gpu_contribution import _small
    r1cs = _small()[0]
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, chains[5][1])
    assert e.value.code == -5 and "serves domains up to 2^5" in str(e.value)
    t = _transcript(7, two=False)
    o = 32
    e3, e5 = t[o + 64 * 3:o + 64 * 4], t[o + 64 * 5:o + 64 * 6]
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, _put(_put(t, o + 64 * 3, e5), o + 64 * 5, e3))
    assert e.value.code == -2 and "step 5" in str(e.value)
