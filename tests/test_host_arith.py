"""CPU: the field/curve templates (csrc/field.hpp, curve.hpp) compiled for the HOST agree with the oracle.

Most of that source is what the gfx950 kernels inline, but not the products of the 8 x 32-bit-limb field: field.hpp chooses by
__HIP_DEVICE_COMPILE__.  Here mul (and so sqr, to_mont, from_mont, inv) is mul_host64, mul_sum2 / mul_sum4 add separate products,
the Fq2 product is Karatsuba and both mul_sub go through those; on the device mul scans product columns in a 96-bit accumulator
(the mac96* asm statements), mul_sum2 / mul_sum4 are one fused scan (field_fused.hpp), the Fq2 product is schoolbook through
mul_sum2 and both mul_sub run the fused sums with negated operands.  zkt_fp and zkt_fq2 below test the host's side of these
only; tests/test_field_raw_cpu.py and tests/test_gpu_field_raw.py run one function (field_raw.hpp) in both builds on raw edge limbs
against integers.  The 29-bit-limb arithmetic further down has its own device hooks (tests/test_gpu_stages.py, test_gpu_group_law.py)."""
import ctypes
import os
import random

import pytest

import bn254 as bn
from bn254 import Q, R
Q_MOD = Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.environ.get("ZKR_HOSTARITH_LIB") or os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "libzkr_hostarith.so")  # the sanitizer run points it at asan/


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SHIM):
        pytest.skip("host arithmetic shim not built (run __graft_entry__.build())")
    return ctypes.CDLL(SHIM)


def _le(v):
    return int(v).to_bytes(32, "little")


def _fp(L, field, op, a, b=0):
    o = ctypes.create_string_buffer(32)
    L.zkt_fp(field, op, _le(a), _le(b), o)
    return int.from_bytes(o.raw, "little")


def test_field_ops(L):
    rnd = random.Random(3)
    for field, P in ((0, Q), (1, R)):
        vals = [0, 1, 2, P - 1, P - 2, 1 << 253, P >> 1] + [rnd.randrange(P) for _ in range(100)]
        for _ in range(300):
            a, b = rnd.choice(vals), rnd.choice(vals)
            assert _fp(L, field, 0, a, b) == a * b % P
            assert _fp(L, field, 1, a, b) == (a + b) % P
            assert _fp(L, field, 2, a, b) == (a - b) % P
            assert _fp(L, field, 4, a) == -a % P
            assert _fp(L, field, 5, a) == a * a % P
        for a in vals[1:20]:
            assert _fp(L, field, 3, a) == pow(a, P - 2, P)


def test_fq2_ops(L):
    rnd = random.Random(4)

    def f2(op, a, b=(0, 0)):
        o = ctypes.create_string_buffer(64)
        L.zkt_fq2(op, _le(a[0]) + _le(a[1]), _le(b[0]) + _le(b[1]), o)
        return (int.from_bytes(o.raw[:32], "little"), int.from_bytes(o.raw[32:], "little"))

    for _ in range(60):
        a, b = (rnd.randrange(Q), rnd.randrange(Q)), (rnd.randrange(Q), rnd.randrange(Q))
        assert f2(0, a, b) == bn.f2mul(a, b) and f2(1, a) == bn.f2sqr(a) and f2(2, a) == bn.f2inv(a)


def test_group_law_including_corner_cases(L):
    rnd = random.Random(5)
    mq = lambda v: _le(v * (1 << 256) % Q)

    def g1mul(P, k):
        o = ctypes.create_string_buffer(64)
        inf = L.zkt_g1_mul(mq(P[0]) + mq(P[1]), _le(k), o)
        return None if inf else (int.from_bytes(o.raw[:32], "little"), int.from_bytes(o.raw[32:], "little"))

    def g2mul(P, k):
        o = ctypes.create_string_buffer(128)
        inf = L.zkt_g2_mul(mq(P[0][0]) + mq(P[0][1]) + mq(P[1][0]) + mq(P[1][1]), _le(k), o)
        v = [int.from_bytes(o.raw[32 * i:32 * i + 32], "little") for i in range(4)]
        return None if inf else ((v[0], v[1]), (v[2], v[3]))

    for k in [1, 2, 3, R - 1, R, R + 1, rnd.randrange(R), (1 << 254) - 1]:
        assert g1mul(bn.G1_GEN, k) == bn.g1_mul(bn.G1_GEN, k)
        assert g2mul(bn.G2_GEN, k) == bn.g2_mul(bn.G2_GEN, k)
    P5 = bn.g1_mul(bn.G1_GEN, 987654321)
    for a, b, ng in [(5, 5, 0), (5, 5, 1), (0, 7, 0), (0, 7, 1), (9, 0, 0), (3, 4, 0), (10, 3, 1), (65535, 65535, 0)]:
        o = ctypes.create_string_buffer(64)
        inf = L.zkt_g1_lincomb(mq(P5[0]) + mq(P5[1]), a, b, ng, o)
        got = None if inf else (int.from_bytes(o.raw[:32], "little"), int.from_bytes(o.raw[32:], "little"))
        assert got == bn.g1_mul(P5, (a + (-b if ng else b)) % R), (a, b, ng)


def test_structured_final_exponentiation_equals_plain_power(L):
    """zkr_verify's final exponentiation (csrc/pairing.hpp: Frobenius maps, three powers by the curve parameter, the
    Scott et al. addition chain) == f^((q^12 - 1)/r) by square-and-multiply, and its Frobenius maps == powers by q."""
    import ctypes
    L.zkt_final_exp_check.argtypes = [ctypes.c_uint64, ctypes.c_int]
    assert L.zkt_final_exp_check(0x5A4B0777, 4) == 4


def test_proof_assembly_multiplications(L):
    """hostops.hpp fixed_base_mul (4-bit window table of delta) and double_scalar_mul (s(A + alfa) + r(B1 + beta) with
    shared doublings) == plain double-and-add, including zero scalars, equal bases and scalars near 2^256."""
    rnd = random.Random(5)
    P = bn.g1_mul(bn.G1_GEN, 7)
    Q = bn.g1_mul(bn.G1_GEN, 1234567)
    wire = lambda pt: _le(pt[0] * (1 << 256) % Q_MOD) + _le(pt[1] * (1 << 256) % Q_MOD)
    cases = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(4)] + [(0, 0), (0, 5), (1, R - 1), ((1 << 256) - 1, 16), (R - 1, R - 1)]
    for a, b in cases:
        assert L.zkt_assembly_muls(wire(P), wire(Q), _le(a), _le(b)) == 1, (a, b)
        assert L.zkt_assembly_muls(wire(P), wire(P), _le(a), _le(b)) == 1, (a, b)      # equal bases: doubling branch of the addition


# ---------------------------------------------------------------- the 29-bit-limb hot-path arithmetic (field29.hpp, curve29.hpp)
def _fp29(L, field, op, a, b=0):
    o = ctypes.create_string_buffer(32)
    L.zkt29_fp(field, op, _le(a), _le(b), o)
    return int.from_bytes(o.raw, "little")


def test_field29_ops_match_the_integers(L):
    """Montgomery products, squares, fused sums of products, lazily reduced additions and subtractions on 9 x 29-bit
    limbs (radix 2^261) against plain integer arithmetic mod q / mod r, including operands at 0, 1, p - 1 and values whose
    limbs are all ones; results come back through the canonical reduction."""
    rnd = random.Random(29)
    for field, P in ((0, Q), (1, R)):
        edge = [0, 1, 2, P - 1, P - 2, (1 << 253) - 1, (1 << 232) - 1, ((1 << 29) - 1) << 29, P >> 1, (1 << 253) + 12345]
        vals = edge + [rnd.randrange(P) for _ in range(60)]
        expect = {
            0: lambda a, b: a * b % P, 1: lambda a, b: a * a % P, 2: lambda a, b: (a + b) % P, 3: lambda a, b: (a - b) % P,
            4: lambda a, b: -a % P, 5: lambda a, b: 0, 6: lambda a, b: (a * a + b * b) % P, 7: lambda a, b: 16 * a * a % P,
            8: lambda a, b: (a * a + b * b) % P, 9: lambda a, b: (a - 3 * b) % P, 10: lambda a, b: -(a - b) ** 2 % P,
            # differences used as product factors WITHOUT their carry sweep (field29.hpp U29; round 3)
            11: lambda a, b: -a * b % P, 12: lambda a, b: b * (a - b) % P, 13: lambda a, b: (a * (a - b) - a * b) % P,
            14: lambda a, b: -a * b % P, 15: lambda a, b: a * b % P,
        }
        for _ in range(400):
            a, b = rnd.choice(vals), rnd.choice(vals)
            for op, fn in expect.items():
                assert _fp29(L, field, op, a, b) == fn(a, b), (field, op, a, b)


def _raw_records(rnd, n):
    """operands as raw limbs: all-ones limbs, single hot limbs, zero, random -- every limb below 2^29"""
    M = (1 << 29) - 1
    pats = [[M] * 9, [0] * 9, [1] + [0] * 8, [0] * 8 + [M], [M] + [0] * 8, [M if i % 2 else 0 for i in range(9)], [M - i for i in range(9)]]
    recs = []
    for k in range(n):
        rec = []
        for _ in range(8):
            rec.append(list(rnd.choice(pats)) if rnd.random() < 0.35 else [rnd.randrange(1 << 29) for _ in range(9)])
        recs.append(rec)
    recs[0] = [[M] * 9] * 8   # the largest column sums the forms can meet
    return recs


# The weight patterns of the sweep-less (U29) factors that the call sites of field29.hpp / curve29.hpp instantiate, per operand
# position a b c d e f g h of a form (1: normalised; 2: neg_loose / cneg_loose, low limbs below 2^30; 3: sub_loose, below 3 * 2^29).
# One factor of every product is normalised and the weight products of a form sum to at most 6 (f29_column_fits: 9 * (1 + 6) = 63
# of the 64 units of 2^58 a column's 64-bit accumulator holds).  The square (form 1) takes normalised operands only.
LOOSE_PATTERNS = (
    (0, (1, 2)),                      # mul(a, neg_loose / cneg_loose): the sign of a table point folded into Y2 ZZZ1
    (0, (1, 3)),                      # mul(a, sub_loose)
    (2, (1, 1, 2, 1)),                # products weighted (1, 2): Fq2 mul / sqr, mul_sub over Fq with a normalised factor
    (2, (1, 3, 2, 1)),                # (3, 2): the Y coordinate over Fq, R (Q - X3) - Y1 P^3
    (2, (1, 2, 1, 2)),                # (2, 2): the Fq2 mul_cneg
    (3, (1, 1, 2, 1, 2, 1, 1, 1)),    # (1, 2, 2, 1): the real part of the Fq2 mul_sub
    (3, (1, 1, 1, 1, 2, 1, 2, 1)),    # (1, 1, 2, 2): its imaginary part
)


def _raw_records_loose(rnd, n):
    """{(form, weights): n records} with the operands of weight 2 / 3 as neg_loose / sub_loose leave them: low eight limbs up to
    2^30 - 1 resp. 3 * 2^29 - 1, top limb below 2^28; the normalised operands as in _raw_records.  Record 0 of every pattern has
    every limb at its ceiling."""
    M = (1 << 29) - 1
    out = {}
    for form, weights in LOOSE_PATTERNS:
        pairs = [weights[i] * weights[i + 1] for i in range(0, len(weights), 2)]
        assert sum(pairs) <= 6 and all(1 in weights[i:i + 2] for i in range(0, len(weights), 2)) and form != 1
        w8 = tuple(weights) + (1,) * (8 - len(weights))
        recs = []
        for k in range(n):
            rec = []
            for w in w8:
                top = (w << 29) - 1
                if w == 1:
                    rec.append([M] * 9 if rnd.random() < 0.3 else [rnd.randrange(1 << 29) for _ in range(9)])
                else:
                    kind = rnd.random()
                    low = [top] * 8 if kind < 0.25 else [top if rnd.random() < 0.5 else rnd.randrange(top + 1) for _ in range(8)] if kind < 0.5 else [rnd.randrange(top + 1) for _ in range(8)]
                    rec.append(low + [rnd.choice([(1 << 28) - 1, rnd.randrange(1 << 28)])])
            recs.append(rec)
        recs[0] = [[M] * 9 if w == 1 else [(w << 29) - 1] * 8 + [(1 << 28) - 1] for w in w8]
        out[(form, weights)] = recs
    return out


def _limbs_value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def raw_forms_host(L, field, form, recs):
    n = len(recs)
    flat = (ctypes.c_uint32 * (72 * n))(*[x for rec in recs for operand in rec for x in operand])
    out = (ctypes.c_uint32 * (9 * n))()
    L.zkt29_raw_forms(field, form, flat, ctypes.c_size_t(n), out)
    return [list(out[9 * k:9 * k + 9]) for k in range(n)]


def test_field29_product_forms_on_raw_limbs(L):
    """The defining recursion of the four Montgomery product forms (field29.hpp mont29) at the limb level, operands not
    reduced at all (every limb up to 2^29 - 1): the result is the sum of products times 2^-261 mod p, its low eight limbs
    are normalised, and it stays below the sum of the operand products / 2^261 + p.  The device's one-statement assembly
    forms are compared with exactly these limbs in tests/test_gpu_stages.py."""
    rnd = random.Random(2929)
    recs = _raw_records(rnd, 200)
    for field, P in ((0, Q), (1, R)):
        rinv = pow(1 << 261, -1, P)
        for form in range(4):
            outs = raw_forms_host(L, field, form, recs)
            for rec, o in zip(recs, outs):
                v = [_limbs_value(x) for x in rec]
                t = [v[0] * v[1], v[0] * v[0], v[0] * v[1] + v[2] * v[3], v[0] * v[1] + v[2] * v[3] + v[4] * v[5] + v[6] * v[7]][form]
                got = _limbs_value(o)
                assert got % P == t * rinv % P, (field, form)
                assert all(x < (1 << 29) for x in o[:8]) and got <= (t >> 261) + P, (field, form)


def test_field29_product_forms_with_loose_factors_at_their_limb_ceilings(L):
    """The same recursion with the factors the group law really feeds it: differences WITHOUT their carry sweep (U29), limbs up to
    2^30 - 1 (neg_loose, cneg_loose) and 3 * 2^29 - 1 (sub_loose), in exactly the weight patterns the call sites instantiate -- up to
    the Fq2 mul_sub's sum of four products with weights 1 + 2 + 2 + 1 = 6, 63 of the 64 units a column may hold.  Agreement with
    Python's integers is what shows that no 64-bit column wrapped; the device's forms are compared with these limbs in
    tests/test_gpu_stages.py."""
    for (form, weights), recs in _raw_records_loose(random.Random(3030), 120).items():
        for field, P in ((0, Q), (1, R)):
            rinv = pow(1 << 261, -1, P)
            outs = raw_forms_host(L, field, form, recs)
            for k, (rec, o) in enumerate(zip(recs, outs)):
                v = [_limbs_value(x) for x in rec]
                t = [v[0] * v[1], None, v[0] * v[1] + v[2] * v[3], v[0] * v[1] + v[2] * v[3] + v[4] * v[5] + v[6] * v[7]][form]
                got = _limbs_value(o)
                assert got % P == t * rinv % P, (field, form, weights, k)
                assert all(x < (1 << 29) for x in o[:8]) and got <= (t >> 261) + P, (field, form, weights, k)


def test_sweepless_differences_on_raw_limbs(L):
    """neg_loose / sub_loose (field29.hpp U29: K p - b and a + K p - b limb by limb against a multiple of p whose low limbs
    were lifted by borrowing, NO carry sweep): for b anywhere below its bound of 13 half moduli (the accumulator's X) and a
    below 4 -- zero, multiples of p and their neighbours, the largest value of the bound, all-ones limbs, random -- every limb
    is non-negative (no wrap), the low eight stay below 2^30 resp. 3 * 2^29 (what the products' column budget assumes), and
    the limbs sum to exactly K p - b resp. a + K p - b."""
    rnd = random.Random(303)
    M = (1 << 29) - 1
    L.zkt29_loose.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.POINTER(ctypes.c_int)] * 2
    for field, P in ((0, Q), (1, R)):
        top_b, top_a = (13 * P) // 2 - 1, 2 * P - 1
        bs = [0, 1, P - 1, P, P + 1, 6 * P, 6 * P + (P >> 1), top_b, top_b - 1, (top_b >> 232) << 232, ((top_b >> 232) << 232) - 1, _limbs_value([M] * 8 + [0])]
        bs += [rnd.randrange(top_b + 1) for _ in range(1500)]
        as_ = [0, 1, top_a, P, _limbs_value([M] * 8 + [0])] + [rnd.randrange(top_a + 1) for _ in range(20)]
        for b in bs:
            a = rnd.choice(as_)
            limbs = lambda v: (ctypes.c_uint32 * 9)(*([(v >> (29 * i)) & M for i in range(8)] + [v >> 232]))
            nl, sl = (ctypes.c_uint32 * 9)(), (ctypes.c_uint32 * 9)()
            kn, ks = ctypes.c_int(), ctypes.c_int()
            L.zkt29_loose(field, limbs(a), limbs(b), nl, sl, ctypes.byref(kn), ctypes.byref(ks))
            assert _limbs_value(nl) == kn.value * P - b and _limbs_value(sl) == a + ks.value * P - b, (field, a, b)
            assert all(x < (1 << 30) for x in nl[:8]) and all(x < 3 << 29 for x in sl[:8]) and nl[8] < (1 << 28) and sl[8] < (1 << 28), (field, a, b)


def test_quotient_estimate_reduction_on_raw_limbs(L):
    """barrett() (the NTT's bound keeper: one quotient estimate from the top limb, no product) and canonical_small():
    for values anywhere below 64 p -- multiples of p and their neighbours, all-ones limbs, random -- the result is congruent,
    non-negative, below 2.5 p, its low limbs normalised; the canonical form is the residue itself."""
    rnd = random.Random(71)
    for field, P in ((0, Q), (1, R)):
        vals = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 63 * P, 64 * P - 1, (1 << 232) - 1, 1 << 232, (P >> 232) << 232]
        vals += [k * P + d for k in (1, 2, 3, 17, 40, 63) for d in (-1, 0, 1, (1 << 232) - 1) if 0 <= k * P + d < 64 * P]
        vals += [rnd.randrange(64 * P) for _ in range(3000)] + [rnd.randrange(4 * P) for _ in range(1000)]
        for v in vals:
            limbs = [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [v >> 232]
            inp = (ctypes.c_uint32 * 9)(*limbs)
            out, can = (ctypes.c_uint32 * 9)(), (ctypes.c_uint32 * 9)()
            L.zkt29_barrett(field, inp, out, can)
            got = _limbs_value(out)
            assert got % P == v % P and 2 * got < 5 * P and all(x < (1 << 29) for x in out[:8]), (field, v)
            assert _limbs_value(can) == v % P, (field, v)


def test_window_table_levels_match_the_oracle(L):
    """The key-load chain (curve29.hpp dbl_jac29 + field29.hpp inv29 with one inversion for all levels, as
    msm_precompute_kernel runs it): 2^(c l) P for l = 1..levels equals the oracle's scalar multiplication, G1 and G2."""
    M = 1 << 256
    for k in (1, 5, 123456789):
        P1 = bn.g1_mul(bn.G1_GEN, k)
        wire = _le(P1[0] * M % Q_MOD) + _le(P1[1] * M % Q_MOD)
        for c, levels in ((3, 5), (7, 12), (20, 2)):
            out = ctypes.create_string_buffer(64 * levels)
            L.zkt29_g1_levels(wire, c, levels, out)
            for l in range(levels):
                e = bn.g1_mul(P1, 1 << (c * (l + 1)))
                assert out.raw[64 * l:64 * l + 64] == _le(e[0]) + _le(e[1]), (k, c, l)
        P2 = bn.g2_mul(bn.G2_GEN, k)
        wire2 = b"".join(_le(v * M % Q_MOD) for v in (P2[0][0], P2[0][1], P2[1][0], P2[1][1]))
        for c, levels in ((4, 6), (20, 2)):
            out = ctypes.create_string_buffer(128 * levels)
            L.zkt29_g2_levels(wire2, c, levels, out)
            for l in range(levels):
                e = bn.g2_mul(P2, 1 << (c * (l + 1)))
                assert out.raw[128 * l:128 * l + 128] == b"".join(_le(v) for v in (e[0][0], e[0][1], e[1][0], e[1][1])), (k, c, l)


def test_radix_change_roundtrip(L):
    """x 2^256 (the key material's Montgomery radix, binarify.ts:78-90) -> x 2^261 (hot-path radix) -> back."""
    rnd = random.Random(31)
    for x in [0, 1, Q - 1] + [rnd.randrange(Q) for _ in range(50)]:
        m256 = x * (1 << 256) % Q
        out, mid = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        L.zkt29_radix_roundtrip(_le(m256), out, mid)
        assert int.from_bytes(mid.raw, "little") == x * (1 << 261) % Q
        assert int.from_bytes(out.raw, "little") == m256


def _wire_g1(P):
    return _le(P[0] * (1 << 256) % Q) + _le(P[1] * (1 << 256) % Q)


def _wire_g2(P):
    return b"".join(_le(c * (1 << 256) % Q) for c in (P[0][0], P[0][1], P[1][0], P[1][1]))


def test_group_law_on_29_bit_limbs_matches_the_oracle(L):
    """add_mixed29 / add_full29 / the doubling and cancellation branches (curve29.hpp) over G1 and G2: signed sums of
    random multiples of the generators -- with repeated points (doubling inside a chain), a point followed by its negative
    (infinity in the middle of a chain), infinity placeholders, and the total added to itself -- equal the oracle's sums."""
    rnd = random.Random(37)
    for g2 in (False, True):
        gen = bn.G2_GEN if g2 else bn.G1_GEN
        mul_ = bn.g2_mul if g2 else bn.g1_mul
        add_ = bn.g2_add if g2 else bn.g1_add
        neg_ = bn.g2_neg if g2 else bn.g1_neg
        wire = _wire_g2 if g2 else _wire_g1
        fn = L.zkt29_g2_chain if g2 else L.zkt29_g1_chain
        pb = 128 if g2 else 64
        base = [mul_(gen, rnd.randrange(1, R)) for _ in range(6)]
        cases = []
        for n in (1, 2, 3, 8, 17):
            pts = [rnd.choice(base) for _ in range(n)]
            cases.append((pts, [rnd.randrange(2) for _ in range(n)]))
        cases.append(([base[0], base[0], base[0], base[1]], [0, 0, 0, 1]))            # the same point three times: doubling inside the chain
        cases.append(([base[2], base[2], base[3], base[3]], [0, 1, 1, 0]))            # P - P: infinity, then Q - Q... total infinity
        cases.append(([base[4], base[4], base[5]], [0, 1, 0]))                        # infinity in the middle, then a point
        cases.append(([base[1], base[1]], [0, 0]))                                    # halves equal: add_full29 doubles
        for pts, signs in cases:
            for twice in (0, 1):
                want = None
                for P, sg in zip(pts, signs):
                    want = add_(want, neg_(P) if sg else P)
                if twice:
                    want = add_(want, want)
                out = ctypes.create_string_buffer(pb)
                blob = b"".join(wire(P) for P in pts)
                inf = fn(blob, bytes(signs), len(pts), twice, out)
                if want is None:
                    assert inf == 1
                else:
                    assert inf == 0
                    got = [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(pb // 32)]
                    flat = [want[0][0], want[0][1], want[1][0], want[1][1]] if g2 else [want[0], want[1]]
                    assert got == flat
        # an all-zero (infinity) wire point inside the list is skipped
        out = ctypes.create_string_buffer(pb)
        assert fn(bytes(pb) + wire(base[0]), bytes([0, 0]), 2, 0, out) == 0


def test_g2_membership_by_endomorphism_equals_the_definition(L):
    """The verifier's G2 membership test psi(Q) == [6x^2]Q (pairing.hpp g2_in_subgroup: a 127-bit multiplication) against the
    definition [r]Q == infinity (g2_in_subgroup_plain) on: multiples of the generator (TxVerifier.sol:30-35), points of the
    twist outside G2, points whose order divides the cofactor 2q - r, and sums of a G2 point with such a point (on the twist,
    outside G2) -- what the bn256 precompile (TxVerifier.sol:91-115) must refuse."""
    import bn254 as b
    from test_abi import _twist_point_outside_g2
    enc = lambda P: b"".join(int(v).to_bytes(32, "little") for v in (P[0][0], P[0][1], P[1][0], P[1][1]))
    P, Pc = _twist_point_outside_g2()
    rnd = random.Random(6)
    inside = [b.g2_mul(b.G2_GEN, k) for k in (1, 2, 3, 0x5A4B, rnd.randrange(b.R), b.R - 1)]
    outside = [P, Pc, b.g2_mul(P, 2, reduce=False), b.g2_mul(P, 7, reduce=False), b.g2_add(inside[3], Pc), b.g2_add(inside[4], P)]
    for Q in inside:
        assert L.zkt_g2_membership(enc(Q)) == 7, Q          # on the twist, in G2 by both tests
    for Q in outside:
        assert b.g2_is_on_curve(Q) and L.zkt_g2_membership(enc(Q)) == 4, Q   # on the twist, refused by both tests


def test_inversion_free_miller_loop_equals_the_affine_one(L):
    """The Miller loop zkr_verify runs (pairing.hpp miller_loop_mixed: homogeneous projective steps for the proof's own G2 point,
    per-key prepared line coefficients for beta / gamma / delta) against the affine loop the earlier rounds pinned to the oracle's
    pairing (multi_miller_loop), after the final exponentiation: random multiples of the generators, every split of three pairs
    into arbitrary and prepared second arguments, a pair with a point at infinity."""
    import bn254 as b
    g1 = b"".join(int(v).to_bytes(32, "little") for v in b.G1_GEN)
    g2 = b"".join(int(v).to_bytes(32, "little") for v in (b.G2_GEN[0][0], b.G2_GEN[0][1], b.G2_GEN[1][0], b.G2_GEN[1][1]))
    L.zkt_miller_loops_agree.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int]
    assert L.zkt_miller_loops_agree(g1, g2, 0x5A4B0999, 3) == 12


def test_shard_group_barrier_and_abort(L):
    """csrc/shard_group.hpp (the barrier of a sharded proof's host threads, zkr_prove.hip calc_h_split): threads pass the
    barriers in step; a thread that fails instead of arriving releases everybody with a refusal, at whatever round."""
    L.zkr_host_shard_group_selftest.restype = ctypes.c_int
    L.zkr_host_shard_group_selftest.argtypes = [ctypes.c_uint] * 4
    for parts in (1, 2, 3, 8):
        assert L.zkr_host_shard_group_selftest(parts, 50, 99, 0) == 0               # nobody fails
        for fail_part in {0, parts - 1}:
            for fail_round in (0, 1, 7, 49):
                assert L.zkr_host_shard_group_selftest(parts, 50, fail_part, fail_round) == 0
