"""Records of raw 32-bit limbs for the 8 x 32-bit-limb field of csrc/field.hpp, and what every operation gives on them as PYTHON
INTEGERS: shared by tests/test_field_raw_cpu.py (host build, libzkr_hostarith.so zkt_fp_raw) and tests/test_gpu_field_raw.py
(device build, zkr_selftest_fp).  Not a test module.  Nothing here calls the shim or an oracle library.

A record is 8 operands of 8 words, least significant word first (csrc/field_raw.hpp); an operation reads the first few and must
ignore the rest, which therefore hold garbage here.  The operations, their numbers and sizes come from csrc/field_raw_ops.def
through zkr_hip.field_raw_ops().  With W = 2^256:
  mul sqr mul_sum2 mul_sum4 mul_sub to_mont from_mont    sum(a_i b_i) / W mod p   (to_mont: b = W^2 mod p; from_mont: b = 1)
  add sub neg                                            the residue
  reduce_once                                            a - p if a >= p else a, as integers
  inv                                                    W^2 / a mod p, inv(0) = 0
  Fq2 ops                                                the same over u^2 = -1, componentwise
All results are canonical: the two builds and the integers agree bit for bit or something is wrong.

Operand ranges are the functions' own (the comments of field.hpp / field_fused.hpp): <= p for the products, mul_sub and neg;
< p for add, sub, inv and the components of Fq2; any 256-bit word for reduce_once.

Per (field, op), in one seeded order: constructed records (a Montgomery quotient of all ones, a quotient of zero, t == p exactly,
column sums at their ceiling, the neg(0) branch, sums at p - 1 / p / p + 1 / 2p - 2), every edge pattern in every operand
position, records drawn from the patterns and random values, and random records -- shuffled, so the lanes of a wavefront take
different branches.  REACH, asserted here from a model of the device's last step (m = T (-1/p) mod W, t = (T + m p) / W): for
every reduction of every product op, both t >= p and t < p occur in at least MIN_REACH records."""
import functools
import random

from bn254 import Q, R
from zkr_hip.binding import FIELD_RAW_RECORD_WORDS, field_raw_ops

W = 1 << 256
M32 = 0xFFFFFFFF
MODULI = (Q, R)
FIELD_NAMES = ("Fq", "Fr")
OPS = field_raw_ops()                       # name -> (number, operands, result words)
OP_NAMES = tuple(sorted(OPS, key=lambda n: OPS[n][0]))
FQ2_OPS = tuple(n for n in OP_NAMES if OPS[n][2] == 16)
PARAMS = [(f, n) for f in (0, 1) for n in OP_NAMES if not (f == 1 and n in FQ2_OPS)]
IDS = ["%s-%s" % (FIELD_NAMES[f], n) for f, n in PARAMS]
INV_OPS = ("inv", "fq2_inv")
PRODUCT_OPS = ("mul", "sqr", "mul_sum2", "mul_sum4", "mul_sub", "to_mont", "from_mont", "fq2_mul", "fq2_sqr", "fq2_mul_sub")
N_RECORDS = 2965                            # 23 workgroups of 128 and 21 lanes: the last wavefront and the last workgroup ragged
N_RECORDS_INV = 197                         # an inversion is about 380 products
MIN_REACH = 64
BATCH_SIZES = (1, 64, 65)                   # a lone lane, a full wavefront, one lane into the next
assert FIELD_RAW_RECORD_WORDS == 64 and len(OP_NAMES) == 16 and OPS["mul"][0] == 0


def bound(p, name):
    """The largest admitted operand."""
    if name == "reduce_once":
        return W - 1
    return p if name in ("mul", "sqr", "mul_sum2", "mul_sum4", "mul_sub", "to_mont", "from_mont", "neg") else p - 1


def top_value(p):
    """The largest value below p whose low seven limbs are all ones."""
    return (((p >> 224) - 1) << 224) | ((1 << 224) - 1)


@functools.lru_cache(maxsize=None)
def patterns(p, hi):
    vals = [0, 1, 2, p - 2, p - 1, p, (p - 1) // 2, (p + 1) // 2, W % p, W * W % p, top_value(p)]
    vals += [1 << (32 * i) for i in range(1, 8)] + [(1 << (32 * i)) - 1 for i in range(1, 8)]
    vals += [M32 << (32 * i) for i in range(8)]
    vals += [sum(M32 << (64 * i) for i in range(4)), sum(M32 << (64 * i + 32) for i in range(4))]
    if hi >= W - 1:                         # reduce_once: around the multiples of p and the top of the word
        vals += [p + 1, 2 * p - 1, 2 * p, 2 * p + 1, 3 * p, 4 * p, 5 * p, 5 * p + 1, 1 << 255, W - 1, W - 2, W - p, (W - 1) // p * p]
    return tuple(sorted(set(v for v in vals if 0 <= v <= hi)))


# ---------------------------------------------------------------- what the operations give, as integers
@functools.lru_cache(maxsize=None)
def _winv(p):
    return pow(W, -1, p)


@functools.lru_cache(maxsize=None)
def _ninv(p):
    return -pow(p, -1, W) % W


def neg_m(p, a):
    return -a % p


def f2mul(p, x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % p, (x[0] * y[1] + x[1] * y[0]) % p)


def expected(p, name, o):
    """The result of operation `name` on the operands o (8 integers), as a tuple of one integer (Fq2: two)."""
    ri = _winv(p)
    if name == "mul": return (o[0] * o[1] * ri % p,)
    if name == "sqr": return (o[0] * o[0] * ri % p,)
    if name == "add": return ((o[0] + o[1]) % p,)
    if name == "sub": return ((o[0] - o[1]) % p,)
    if name == "neg": return (-o[0] % p,)
    if name == "reduce_once": return (o[0] - p if o[0] >= p else o[0],)
    if name == "mul_sum2": return ((o[0] * o[1] + o[2] * o[3]) * ri % p,)
    if name == "mul_sum4": return ((o[0] * o[1] + o[2] * o[3] + o[4] * o[5] + o[6] * o[7]) * ri % p,)
    if name == "mul_sub": return ((o[0] * o[1] - o[2] * o[3]) * ri % p,)
    if name == "to_mont": return (o[0] * (W * W % p) * ri % p,)
    if name == "from_mont": return (o[0] * ri % p,)
    if name == "inv": return (pow(o[0], -1, p) * W * W % p if o[0] % p else 0,)
    x, y, z, w = (o[0], o[1]), (o[2], o[3]), (o[4], o[5]), (o[6], o[7])
    if name == "fq2_mul":
        r = f2mul(p, x, y)
    elif name == "fq2_sqr":
        r = f2mul(p, x, x)
    elif name == "fq2_mul_sub":
        a, b = f2mul(p, x, y), f2mul(p, z, w)
        r = ((a[0] - b[0]) % p, (a[1] - b[1]) % p)
    else:
        assert name == "fq2_inv"
        n = (x[0] * x[0] + x[1] * x[1]) % p
        if n == 0:
            assert x == (0, 0)              # -1 is no square mod q
            return (0, 0)
        ni = pow(n, -1, p) * W * W % p
        return (x[0] * ni % p, -x[1] * ni % p)
    return tuple(v * ri % p for v in r)


# ---------------------------------------------------------------- the device's last step, for the reach of the records
def redc(p, T):
    """(t, m) of the Montgomery reduction of the column sum T: m = T (-1/p) mod W, t = (T + m p) / W, before the last subtraction."""
    m = T * _ninv(p) % W
    t, rem = divmod(T + m * p, W)
    assert rem == 0
    return t, m


def neg_dev(p, a):
    """neg() as the code has it: zero stays zero, anything else (p included) becomes p - a."""
    return 0 if a == 0 else p - a


def device_sums(p, name, o):
    """The sums of products T that the DEVICE build reduces for one record, one per reduction."""
    if name == "mul": return [o[0] * o[1]]
    if name == "sqr": return [o[0] * o[0]]
    if name == "mul_sum2": return [o[0] * o[1] + o[2] * o[3]]
    if name == "mul_sum4": return [o[0] * o[1] + o[2] * o[3] + o[4] * o[5] + o[6] * o[7]]
    if name == "mul_sub": return [o[0] * o[1] + neg_dev(p, o[2]) * o[3]]
    if name == "to_mont": return [o[0] * (W * W % p)]
    if name == "from_mont": return [o[0]]
    xa, xb, ya, yb, za, zb, wa, wb = o
    if name == "fq2_mul": return [xa * ya + neg_dev(p, xb) * yb, xa * yb + xb * ya]
    if name == "fq2_sqr": return [xa * xb, (xa + xb) % p * ((xa - xb) % p)]
    assert name == "fq2_mul_sub"
    nza = neg_dev(p, za)
    return [xa * ya + neg_dev(p, xb) * yb + nza * wa + zb * wb, xa * yb + xb * ya + nza * wb + neg_dev(p, zb) * wa]


def device_model(p, name, o):
    """(result, [t >= p for every reduction]) of a product op through the model of the device's steps."""
    ts = [redc(p, T)[0] for T in device_sums(p, name, o)]
    assert all(t < 2 * p for t in ts), name
    red = [t - p if t >= p else t for t in ts]
    if name == "fq2_sqr":
        red = [red[1], 2 * red[0] % p]      # ((a + b)(a - b), 2 a b)
    return tuple(red), [t >= p for t in ts]


def inv_model(p, a, flags):
    """inv_inline of field.hpp: a^(p - 2) in Montgomery form, least significant exponent bit first; appends t >= p of every product."""
    def mont(x, y):
        t = redc(p, x * y)[0]
        flags.append(t >= p)
        return t - p if t >= p else t
    r, b, e = W % p, a, p - 2
    for _ in range(254):
        if e & 1:
            r = mont(r, b)
        b = mont(b, b)
        e >>= 1
    assert e == 0
    return r


def inv_device_model(p, name, o):
    flags = []
    if name == "inv":
        return (inv_model(p, o[0], flags),), flags
    def mont(x, y):
        t = redc(p, x * y)[0]
        flags.append(t >= p)
        return t - p if t >= p else t
    n = inv_model(p, (mont(o[0], o[0]) + mont(o[1], o[1])) % p, flags)
    return (mont(o[0], n), neg_dev(p, mont(o[1], n))), flags


# ---------------------------------------------------------------- the records
class Cases:
    """The records of one (field, op) in their final order: operands (8 integers each, garbage past the op's count), kinds, the
    integers every result must equal, and the bytes both builds read."""

    def __init__(self, field, name):
        self.field, self.name, self.p = field, name, MODULI[field]
        self.num, self.n_in, self.out_words = OPS[name]
        self.n_out = self.out_words // 8
        self.hi = bound(self.p, name)
        self.rnd = random.Random(0xF1E1D000 + 64 * field + self.num)
        self.pats = patterns(self.p, self.hi)
        n_total = N_RECORDS_INV if name in INV_OPS else N_RECORDS
        recs = self._constructed()
        self.n_constructed = len(recs)
        recs += [("pattern", [v] * self.n_in) for v in self.pats]
        if self.n_in == 2:                  # two operands: every pair of the leading patterns as well
            lead = [v for v in (0, 1, 2, self.p - 2, self.p - 1, self.p, (self.p + 1) // 2, top_value(self.p)) if v <= self.hi]
            recs += [("pattern", [a, b]) for a in lead for b in lead]
        if name in PRODUCT_OPS:
            recs += self._reach_records()
        n_mixed = (n_total - len(recs)) * 3 // 5
        assert n_mixed > 0, (name, len(recs))
        recs += [("mixed", self._draw(0.7)) for _ in range(n_mixed)]
        recs += [("random", self._draw(0.0)) for _ in range(n_total - len(recs))]
        head = recs[:self.n_constructed]
        self.rnd.shuffle(head)
        # the batches: the constructed records first, the patterns behind them where an op has fewer than a wavefront and a lane
        self.batch_recs = [self._finish(k, o) for k, o in (head + recs[self.n_constructed:])[:max(BATCH_SIZES)]]
        self.rnd.shuffle(recs)
        done = [self._finish(k, o) for k, o in recs]
        self.kinds = [d[0] for d in done]
        self.ops = [d[1] for d in done]
        self.want = [expected(self.p, name, o) for o in self.ops]
        self.data = self.pack(self.ops)
        assert len(self.ops) == n_total and len(self.data) == 256 * n_total
        self._self_check()

    # -- helpers
    def _rand(self):
        return self.rnd.randrange(self.hi + 1)

    def _draw(self, p_edge):
        return [self.rnd.choice(self.pats) if self.rnd.random() < p_edge else self._rand() for _ in range(self.n_in)]

    def _finish(self, kind, o):
        o = list(o)
        assert len(o) == self.n_in and all(0 <= v <= self.hi for v in o), (self.name, kind, o)
        return kind, tuple(o + [self.rnd.randrange(W) for _ in range(8 - self.n_in)])   # what the op must not read

    @staticmethod
    def pack(ops):
        return b"".join(v.to_bytes(32, "little") for o in ops for v in o)

    def batch(self, n):
        """(bytes of the first n batch records, their kinds, operands and expected integers)."""
        part = self.batch_recs[:n]
        ops = [o for _, o in part]
        return self.pack(ops), [k for k, _ in part], ops, [expected(self.p, self.name, o) for o in ops]

    def _reach_records(self):
        """For every reduction of the op: MIN_REACH + 16 records with t >= p and as many with t < p, taken from the mixed draws."""
        out = []
        n_slots = len(device_sums(self.p, self.name, [1] * 8))
        for slot in range(n_slots):
            for want_ge in (True, False):
                got = 0
                while got < MIN_REACH + 16:
                    o = self._draw(0.7 if self.name == "from_mont" else 0.35)
                    if (redc(self.p, device_sums(self.p, self.name, o + [0] * (8 - self.n_in))[slot])[0] >= self.p) == want_ge:
                        out.append(("reach", o))
                        got += 1
        return out

    # -- the constructed records of the op
    def _constructed(self):
        p, name, rnd = self.p, self.name, self.rnd
        top = top_value(p)
        rb = lambda: rnd.randrange(p)                      # a canonical value
        out = []
        add = lambda kind, o: out.append((kind, list(o)))
        pairs = {"mul": 1, "mul_sum2": 2, "mul_sum4": 4}.get(name)
        if pairs:
            # quotient all ones: the sum of products = p mod W, solved for the second operand of one pair
            for pos in range(pairs):
                found = 0
                while found < (16 if pairs == 1 else 8):
                    o = [rb() for _ in range(2 * pairs)]
                    o[2 * pos] |= 1
                    if o[2 * pos] > p:
                        continue
                    rest = sum(o[2 * k] * o[2 * k + 1] for k in range(pairs) if k != pos)
                    o[2 * pos + 1] = (p - rest) * pow(o[2 * pos], -1, W) % W
                    if o[2 * pos + 1] <= p:
                        assert redc(p, sum(o[2 * k] * o[2 * k + 1] for k in range(pairs)))[1] == W - 1
                        add("quotient all ones", o)
                        found += 1
                o = [0] * (2 * pairs)
                o[2 * pos], o[2 * pos + 1] = 1, p
                add("quotient all ones", o)                 # 1 x p: result 0
                o = [0] * (2 * pairs)
                o[2 * pos], o[2 * pos + 1] = p, 1
                add("quotient all ones", o)
                # quotient zero: 2^(32 k) x 2^(256 - 32 k) = W, result 1
                for k in range(1, 8):
                    for swap in (0, 1):
                        o = [0] * (2 * pairs)
                        o[2 * pos + swap], o[2 * pos + 1 - swap] = 1 << (32 * k), 1 << (256 - 32 * k)
                        for j in range(pairs):              # the other pairs: a zero factor beside anything
                            if j != pos:
                                o[2 * j + rnd.randrange(2)] = rnd.choice((0, p, top, rb()))
                        assert sum(o[2 * j] * o[2 * j + 1] for j in range(pairs)) == W and redc(p, W) == (1, 0)
                        add("quotient zero", o)
                # t == p exactly: a multiple of p as the sum
                for b in (1, 2, p - 1, p, rb(), rb()):
                    for swap in (0, 1):
                        o = [0] * (2 * pairs)
                        o[2 * pos + swap], o[2 * pos + 1 - swap] = p, b
                        for j in range(pairs):
                            if j != pos and rnd.randrange(2):
                                o[2 * j], o[2 * j + 1] = p, rnd.choice((1, p - 1, p, rb()))
                        add("t == p", o)
            add("t == p", [p] * (2 * pairs))
            add("ceiling columns", [top] * (2 * pairs))
            for _ in range(4):
                add("ceiling columns", [rnd.choice((top, p, p - 1)) for _ in range(2 * pairs)])
        elif name == "sqr":
            for v in (p, top, 1 << 128, 0, 1, p - 1, (1 << 128) - 1, (1 << 128) + 1):
                add({p: "t == p", top: "ceiling columns", 1 << 128: "quotient zero"}.get(v, "edge"), [v])
        elif name in ("to_mont", "from_mont"):
            r2 = W * W % p
            for v in (p, 0, 1, top, pow(r2, -1, p), W % p, r2):
                add("t == p" if v == p else "edge", [v])
            a = p * pow(r2 if name == "to_mont" else 1, -1, W) % W
            if a <= p:
                add("quotient all ones", [a])
            if name == "from_mont":                          # the only operand whose t reaches p is p itself
                out += [("t == p", [p])] * 8
        elif name == "mul_sub":
            for _ in range(8):
                a, b, c, d = rb(), rb(), rb(), rb()
                add("neg(0)", [a, b, 0, d]); add("neg(0)", [a, b, c, 0]); add("neg(0)", [a, b, 0, 0]); add("neg(0)", [a, b, p, d])
                add("a b == c d", [a, b, a, b]); add("a b == c d", [a, b, b, a])
                add("t == p", [p, b, 0, d]); add("t == p", [p, b, c, 0]); add("t == p", [a, p, p, d])
                add("ordinary", [a, b, c, d])
            for k in range(1, 8):
                add("quotient zero", [1 << (32 * k), 1 << (256 - 32 * k), 0, rb()])
                add("quotient zero", [1 << (32 * k), 1 << (256 - 32 * k), rb(), 0])
            add("ceiling columns", [top, top, top, top]); add("ceiling columns", [top, top, p - top, top]); add("t == p", [p, p, p, p])
            add("a b == c d", [0, 0, 0, 0]); add("a b == c d", [p, p - 1, p - 1, p])
        elif name == "add":
            for s in (p - 1, p, p + 1, 2 * p - 2):
                for _ in range(8):
                    a = rnd.randrange(max(0, s - (p - 1)), min(p - 1, s) + 1)
                    add("a + b = p%+d" % (s - p) if s < 2 * p - 2 else "a + b = 2p - 2", [a, s - a])
                for a in (0, 1, p - 1, (p - 1) // 2, (p + 1) // 2):
                    if 0 <= s - a <= p - 1:
                        add("a + b = p%+d" % (s - p) if s < 2 * p - 2 else "a + b = 2p - 2", [a, s - a])
        elif name == "sub":
            for _ in range(8):
                a = rb()
                add("a == b", [a, a]); add("a = 0", [0, rb()]); add("b = p - 1", [rb(), p - 1]); add("a = b - 1", [a, a + 1] if a + 1 < p else [0, 1])
            add("a == b", [0, 0]); add("a == b", [p - 1, p - 1]); add("a = 0", [0, p - 1]); add("a = 0", [0, 1]); add("b = p - 1", [p - 1, p - 1]); add("b = p - 1", [p - 2, p - 1])
        elif name == "neg":
            for v in (0, p, 1, p - 1, 2, p - 2, top, 1 << 224, (1 << 224) - 1):
                add("neg(0)" if v in (0, p) else "edge", [v])
        elif name == "reduce_once":
            for v in (0, p - 1, p, p + 1, 2 * p - 1, 2 * p, W - 1, 1 << 255, p ^ 1, p - (1 << 224), p + (1 << 224), p - (1 << 32), p + (1 << 32)):
                add("edge", [v])
            for i in range(8):                              # the borrow decided in limb i: equal above, one less / one more there
                add("borrow in limb %d" % i, [p - (1 << (32 * i))]); add("borrow in limb %d" % i, [(p >> (32 * i) << (32 * i))])
        elif name == "inv":
            for v in (0, 1, W % p, p - 1, W * W % p, 2, p - 2, top):
                add("edge", [v])
        elif name == "fq2_mul":
            for _ in range(8):
                xa, xb, ya, yb = rb(), rb(), rb(), rb()
                add("neg(0)", [xa, 0, ya, yb]); add("conjugate", [xa, xb, xa, neg_m(p, xb)]); add("neg(0)", [0, 0, ya, yb]); add("ordinary", [xa, xb, ya, yb])
                add("neg(0)", [xa, 0, ya, 0]); add("conjugate", [xa, neg_m(p, xb), xa, xb]); add("edge", [xa, xb, 0, 0]); add("edge", [0, xb, 0, yb])
            for k in range(1, 8):
                add("quotient zero", [1 << (32 * k), 0, 1 << (256 - 32 * k), 0]); add("quotient zero", [1 << (32 * k), 0, 0, 1 << (256 - 32 * k)])
            add("ceiling columns", [top] * 4); add("ceiling columns", [top, p - top, top, top]); add("ceiling columns", [p - 1] * 4); add("edge", [p - 1, 1, p - 1, 1])
        elif name == "fq2_sqr":
            for _ in range(8):
                a = rb()
                add("a == b", [a, a]); add("a == p - b", [a, neg_m(p, a)]); add("b = 0", [a, 0]); add("a = 0", [0, a]); add("ordinary", [a, rb()])
            for v in (0, 1, p - 1, top, (p - 1) // 2, (p + 1) // 2):
                add("a == b", [v, v]); add("a == p - b", [v, neg_m(p, v)])
            add("a == p - b", [(p + 1) // 2, (p - 1) // 2]); add("quotient zero", [1 << 128, 1 << 128]); add("ceiling columns", [top, top - 1])
        elif name == "fq2_mul_sub":
            for _ in range(8):
                x, y, z, w = [rb(), rb()], [rb(), rb()], [rb(), rb()], [rb(), rb()]
                add("neg(0): z.a = 0", x + y + [0, z[1]] + w); add("neg(0): z.b = 0", x + y + [z[0], 0] + w); add("neg(0): z = 0", x + y + [0, 0] + w)
                add("x y == z w", x + y + x + y); add("x y == z w", x + y + y + x); add("neg(0): x.b = 0", [x[0], 0] + y + z + w); add("ordinary", x + y + z + w)
            add("ceiling columns", [top] * 8); add("ceiling columns", [top, p - top, top, top, p - top, p - top, top, top]); add("ceiling columns", [p - 1] * 8)
            add("x y == z w", [0] * 8); add("neg(0): z = 0", [p - 1, p - 1, p - 1, p - 1, 0, 0, p - 1, p - 1])
        elif name == "fq2_inv":
            for v in ((0, 0), (1, 0), (0, 1), (W % p, 0), (0, W % p), (p - 1, p - 1), (p - 1, 0), (0, p - 1), (1, 1), (top, top), (rb(), 0), (0, rb())):
                add("edge", list(v))
        return out

    # -- what the list promises
    def _self_check(self):
        p, name = self.p, self.name
        model = device_model if name in PRODUCT_OPS else inv_device_model if name in INV_OPS else None
        self.reach = None
        if model:
            flags = []
            for o, w in zip(self.ops, self.want):
                res, f = model(p, name, o)
                assert res == w, (name, o)              # the model of the device's steps and the plain integers agree
                flags.append(f)
            if name in INV_OPS:                         # a chain of products per record: records in which each outcome occurs
                self.reach = [(sum(1 for f in flags if any(f)), sum(1 for f in flags if not all(f)))]
            else:
                self.reach = [(sum(1 for f in flags if f[s]), sum(1 for f in flags if not f[s])) for s in range(len(flags[0]))]
        for w in self.want:
            assert len(w) == self.n_out and all(0 <= v < (W if name == "reduce_once" else p) for v in w)
        if name in ("mul", "mul_sum2", "mul_sum4"):
            for kind in ("quotient all ones", "quotient zero", "t == p", "ceiling columns"):
                assert self.kinds.count(kind) >= 5, (name, kind)
            pairs = self.n_in // 2
            for kind, o in zip(self.kinds, self.ops):
                t, m = redc(p, sum(o[2 * k] * o[2 * k + 1] for k in range(pairs)))
                assert (kind != "quotient all ones" or m == W - 1) and (kind != "quotient zero" or (m == 0 and t == 1)) and (kind != "t == p" or t == p)
        if name in ("mul_sub", "fq2_mul", "fq2_mul_sub"):
            assert sum(k.startswith("neg(0)") for k in self.kinds) >= 16
            for kind, w in zip(self.kinds, self.want):
                assert kind not in ("a b == c d", "x y == z w") or not any(w)
                assert kind != "conjugate" or w[1] == 0


@functools.lru_cache(maxsize=None)
def cases(field, name):
    return Cases(field, name)


# ---------------------------------------------------------------- comparing a build's bytes with the integers
def ints(data, n_out):
    """Result bytes -> one tuple of n_out integers per record."""
    step = 32 * n_out
    assert len(data) % step == 0
    return [tuple(int.from_bytes(data[i + 32 * j:i + 32 * j + 32], "little") for j in range(n_out)) for i in range(0, len(data), step)]


def describe(cs, i, kind, o):
    return "%s %s record %d (%s), operands %s" % (FIELD_NAMES[cs.field], cs.name, i, kind, " ".join("%064x" % v for v in o[:cs.n_in]))


def check_against(cs, got_bytes, want, kinds, ops, who, what="the integers"):
    """Every record of `got_bytes` (a build's result) equals `want` (tuples of integers); the first difference is named with its
    record, kind and operands.  Returns the number of records compared."""
    got = ints(got_bytes, cs.n_out)
    assert len(got) == len(want), "%s: %d results for %d records" % (who, len(got), len(want))
    if got != want:
        bad = [i for i in range(len(want)) if got[i] != want[i]]
        i = bad[0]
        raise AssertionError("%s differs from %s in %d of %d records, first: %s: got %s, want %s; kinds of the first ones: %s" % (
            who, what, len(bad), len(want), describe(cs, i, kinds[i], ops[i]), " ".join("%064x" % v for v in got[i]),
            " ".join("%064x" % v for v in want[i]), sorted(set(kinds[j] for j in bad[:64]))))
    return len(want)
