"""Records of raw 29-bit limbs for the group law of csrc/curve29.hpp, and the integer model of each operation: shared by
tests/test_group_law_bounds_cpu.py (host build, libzkr_hostarith.so zkt29_curve_raw), tests/test_gpu_group_law.py (device build,
zkr_selftest_curve29) and tests/test_chain_forms_cpu.py (the affine + affine and affine doubling models).

A coordinate is 9 limbs over Fq (G1) and 18 over Fq2 (G2: re, im): the low eight below 2^29, the top limb = value >> 232; values
are x 2^261 mod q plus any multiple of q the coordinate's bound admits.  A record is the operation's coordinates, then two flag
words (csrc/curve29_raw.hpp).  The model decodes with 2^-261 and works mod q with oracle/bn254.py.

Three families per operation and group:
  * coordinates AT the limits of their declared bounds -- no points of the curve: the forms are polynomial identities -- and
    random ones: 0, 1, q - 1, every k q and k q +- 1 below the bound, the last values below it, all-ones low limbs;
  * points of the curve in non-canonical clothes, (l^2 x + k1 q, l^3 y + k2 q, l^2 + k3 q, l^3 + k4 q), against themselves, their
    negatives, other points and infinity: expected from the oracle's group law;
  * over Fq2, x differences (t, +-t): the real part of their square is exactly zero while the square is not, so the cheap zero
    test (maybe_zero_mod_p: limb 0 of the real part) passes and the full one has to refuse.
Every record's branch (general, doubling, cancellation, infinity operand) is the MODEL's; the order puts every branch into every
full wavefront of 64, then one wavefront all general and one all doubling, then a ragged tail."""
import functools
import random

import bn254 as bn
from bn254 import Q

M29 = (1 << 29) - 1
RADIX = 1 << 261
RINV = pow(RADIX, -1, Q)
HX, HY = 13, 4                      # curve29.hpp XYZZ29: X below 13 half moduli, Y ZZ ZZZ below 4
JX, JY, JZ = 5, 5, 8                # Jac29
N_RECORDS = 2048 + 37               # the tail leaves the last workgroup (128) and the last wavefront (64) ragged
N_MIXED = 30                        # wavefronts that hold every branch; then one all general, one all doubling (or general)
OPS = tuple(range(7))
OP_NAMES = ("add_mixed29", "add_affine_affine29", "add_full29", "dbl_xyzz29", "dbl_affine29", "dbl_jac29", "pack_xyzz/unpack_xyzz")
XYZZ_B = (HX, HY, HY, HY)
IN_BOUNDS = (XYZZ_B + (2, 2), (2, 2, 2, 2), XYZZ_B + XYZZ_B, XYZZ_B, (2, 2), (JX, JY, JZ), XYZZ_B)
OUT_BOUNDS = (XYZZ_B, XYZZ_B, XYZZ_B, XYZZ_B, XYZZ_B, (JX, JY, JZ), XYZZ_B)
# coordinates that are never congruent to zero for a finite point: y, ZZ (and the Jacobian Y, Z)
NONZERO = ((1, 2, 5), (1, 3), (1, 2, 5, 6), (1, 2), (1,), (1, 2), (1, 2))
BRANCHES = (("general", "dbl", "cancel", "inf"), ("general", "dbl", "cancel"), ("general", "dbl", "cancel", "inf"), ("general", "inf"),
            ("general",), ("general",), ("general", "inf"))


class F1:
    """Fq as integers."""
    g2, size = 0, 32
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b % Q)
    neg = staticmethod(lambda a: -a % Q)
    inv = staticmethod(lambda a: pow(a, Q - 2, Q))
    enc = staticmethod(lambda a: int(a).to_bytes(32, "little"))
    dec = staticmethod(lambda b: int.from_bytes(b, "little"))
    rand = staticmethod(lambda rnd: rnd.randrange(Q))
    edges = [0, 1, 2, Q - 1, Q - 2, Q >> 1, (1 << 253) - 1, ((1 << 254) - 1) % Q, int("1" * 254, 2) % Q]
    gen, padd, pmul, pneg = bn.G1_GEN, staticmethod(bn.g1_add), staticmethod(bn.g1_mul), staticmethod(bn.g1_neg)
    # raw coordinates (any representative) <-> field elements
    comps = staticmethod(lambda v: (v,))
    join = staticmethod(lambda c: c[0])
    scal = staticmethod(lambda a, k: a * k % Q)


class F2:
    """Fq2 as pairs (re, im)."""
    g2, size = 1, 64
    zero, one = (0, 0), (1, 0)
    add, sub, mul, neg, inv = (staticmethod(f) for f in (bn.f2add, bn.f2sub, bn.f2mul, bn.f2neg, bn.f2inv))
    enc = staticmethod(lambda a: int(a[0]).to_bytes(32, "little") + int(a[1]).to_bytes(32, "little"))
    dec = staticmethod(lambda b: (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")))
    rand = staticmethod(lambda rnd: (rnd.randrange(Q), rnd.randrange(Q)))
    edges = [(0, 0), (1, 0), (0, 1), (Q - 1, Q - 1), (Q - 1, 0), (0, Q - 1), (Q - 2, 1), (Q >> 1, (1 << 253) - 1)]
    gen, padd, pmul, pneg = bn.G2_GEN, staticmethod(bn.g2_add), staticmethod(bn.g2_mul), staticmethod(bn.g2_neg)
    comps = staticmethod(lambda v: tuple(v))
    join = staticmethod(lambda c: (c[0], c[1]))
    scal = staticmethod(lambda a, k: (a[0] * k % Q, a[1] * k % Q))


FIELDS = (F1, F2)


# ---------------------------------------------------------------- the formulas of curve29.hpp on integers
def dbl_affine_model(F, x, y):
    u = F.add(y, y); v = F.mul(u, u); w = F.mul(u, v); s = F.mul(x, v)
    xx = F.mul(x, x); m = F.add(F.add(xx, xx), xx)
    x3 = F.sub(F.mul(m, m), F.add(s, s))
    return x3, F.sub(F.mul(m, F.sub(s, x3)), F.mul(w, y)), v, w


def affine_affine_model(F, a, neg_a, b, neg_b):
    """The formulas of add_affine_affine29 on integers, special cases included."""
    x1, y1 = a[0], F.neg(a[1]) if neg_a else a[1]
    x2, y2 = b[0], F.neg(b[1]) if neg_b else b[1]
    p, r = F.sub(x2, x1), F.sub(y2, y1)
    if p == F.zero:
        return dbl_affine_model(F, x1, y1) if r == F.zero else None
    pp = F.mul(p, p); ppp = F.mul(p, pp); q = F.mul(x1, pp)
    x3 = F.sub(F.sub(F.mul(r, r), ppp), F.add(q, q))
    return x3, F.sub(F.mul(r, F.sub(q, x3)), F.mul(y1, ppp)), pp, ppp


def dbl_xyzz_model(F, p):
    x3, y3, v, w = dbl_affine_model(F, p[0], p[1])
    return x3, y3, F.mul(v, p[2]), F.mul(w, p[3])


def _general_add(F, u1, u2, s1, s2, zz, zzz):
    """X3 Y3 ZZ3 ZZZ3 from U1 U2 S1 S2 and the product of the operands' ZZ / ZZZ; None when the x difference vanishes."""
    p, r = F.sub(u2, u1), F.sub(s2, s1)
    if p == F.zero:
        return None, r == F.zero
    pp = F.mul(p, p); ppp = F.mul(p, pp); q = F.mul(u1, pp)
    x3 = F.sub(F.sub(F.mul(r, r), ppp), F.add(q, q))
    return (x3, F.sub(F.mul(r, F.sub(q, x3)), F.mul(s1, ppp)), F.mul(zz, pp), F.mul(zzz, ppp)), False


def add_mixed_model(F, acc, q, neg_q):
    x, y = q[0], F.neg(q[1]) if neg_q else q[1]
    res, same = _general_add(F, acc[0], F.mul(x, acc[2]), acc[1], F.mul(y, acc[3]), acc[2], acc[3])
    if res is not None:
        return res, "general"
    return (dbl_affine_model(F, x, y), "dbl") if same else (None, "cancel")


def add_full_model(F, a, b):
    res, same = _general_add(F, F.mul(a[0], b[2]), F.mul(b[0], a[2]), F.mul(a[1], b[3]), F.mul(b[1], a[3]), F.mul(a[2], b[2]), F.mul(a[3], b[3]))
    if res is not None:
        return res, "general"
    return (dbl_xyzz_model(F, b), "dbl") if same else (None, "cancel")


def dbl_jac_model(F, p):
    """dbl-2009-l with a = 0: E = 3 X^2, S = 4 X Y^2, X3 = E^2 - 2 S, Y3 = E (S - X3) - 8 Y^4, Z3 = 2 Y Z."""
    X, Y, Z = p
    yy = F.mul(Y, Y)
    e = F.scal(F.mul(X, X), 3); s = F.scal(F.mul(X, yy), 4)
    x3 = F.sub(F.mul(e, e), F.add(s, s))
    return x3, F.sub(F.mul(e, F.sub(s, x3)), F.scal(F.mul(yy, yy), 8)), F.scal(F.mul(Y, Z), 2)


def decode(F, raw):
    """A raw coordinate (any representative, x 2^261) as a field element."""
    return F.join(tuple(c * RINV % Q for c in F.comps(raw)))


def is_zero_raw(F, raw):
    return all(c == 0 for c in F.comps(raw))


def model(F, op, coords, flags):
    """(result, branch) of operation `op` on raw coordinates: result = tuple of field elements (standard form), None = infinity."""
    v = [decode(F, c) for c in coords]
    if op == 0:
        if is_zero_raw(F, coords[2]):
            return (v[4], F.neg(v[5]) if flags[0] else v[5], F.one, F.one), "inf"
        return add_mixed_model(F, v[0:4], v[4:6], flags[0])
    if op == 1:
        x1, y1 = v[0], F.neg(v[1]) if flags[0] else v[1]
        x2, y2 = v[2], F.neg(v[3]) if flags[1] else v[3]
        branch = "general" if x1 != x2 else "dbl" if y1 == y2 else "cancel"
        return affine_affine_model(F, v[0:2], flags[0], v[2:4], flags[1]), branch
    if op == 2:
        a_inf, b_inf = is_zero_raw(F, coords[2]), is_zero_raw(F, coords[6])
        if a_inf or b_inf:
            return (None if (a_inf and b_inf) else tuple(v[4:8]) if a_inf else tuple(v[0:4])), "inf"
        return add_full_model(F, v[0:4], v[4:8])
    if op == 3:
        return (None, "inf") if is_zero_raw(F, coords[2]) else (dbl_xyzz_model(F, v), "general")
    if op == 4:
        return dbl_affine_model(F, v[0], v[1]), "general"
    if op == 5:
        return dbl_jac_model(F, v), "general"
    return (None, "inf") if is_zero_raw(F, coords[2]) else (tuple(v), "general")


def to_affine(F, P):
    """XYZZ (X, Y, ZZ, ZZZ) or Jacobian (X, Y, Z) as the affine point; None stays None."""
    if P is None:
        return None
    if len(P) == 3:
        zi = F.inv(P[2]); zi2 = F.mul(zi, zi)
        return F.mul(P[0], zi2), F.mul(P[1], F.mul(zi2, zi))
    return F.mul(P[0], F.inv(P[2])), F.mul(P[1], F.inv(P[3]))


# ---------------------------------------------------------------- values at the limits of a bound
def max_value(H):
    return (H * Q - 1) // 2            # the largest value below H q / 2


@functools.lru_cache(maxsize=None)
def edge_values(H, nonzero):
    top, fl = max_value(H), H * Q // 2
    all_ones = ((((top + 1) >> 232) - 1) << 232) + (1 << 232) - 1   # the largest value below the bound whose low eight limbs are all 2^29 - 1
    vals = {0, 1, Q - 1, Q, Q + 1, fl - 1, fl - 2, top, all_ones}
    for k in range(0, H // 2 + 2):
        vals |= {k * Q - 1, k * Q, k * Q + 1}
    return tuple(sorted(v for v in vals if 0 <= v <= top and not (nonzero and v % Q == 0)))


def _pick(rnd, H, nonzero, p_edge=0.65):
    if rnd.random() < p_edge:
        return rnd.choice(edge_values(H, nonzero))
    while True:
        v = rnd.randrange(max_value(H) + 1)
        if not (nonzero and v % Q == 0):
            return v


def pick_coord(F, rnd, H, nonzero, p_edge=0.65):
    """One raw coordinate below H half moduli (per component); never congruent to zero where `nonzero`."""
    if not F.g2:
        return _pick(rnd, H, nonzero, p_edge)
    a = _pick(rnd, H, False, p_edge)
    return a, _pick(rnd, H, nonzero and a % Q == 0, p_edge)


def lift(F, rnd, val, H, how=None):
    """The field element `val` as a raw coordinate: x 2^261 mod q, plus a multiple of q -- none, the most the bound admits, or any."""
    out = []
    for c in F.comps(val):
        m = c * RADIX % Q
        kmax = (max_value(H) - m) // Q
        out.append(m + Q * {"low": 0, "high": kmax, None: rnd.choice((0, kmax, rnd.randrange(kmax + 1)))}[how])
    return F.join(tuple(out))


def limbs(v):
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def limbs_value(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


class Record:
    __slots__ = ("coords", "flags", "family", "expect", "has_expect")

    def __init__(self, coords, flags=(0, 0), family="", expect=None, has_expect=False):
        self.coords, self.flags, self.family, self.expect, self.has_expect = tuple(coords), tuple(flags), family, expect, has_expect

    def words(self, F):
        w = []
        for c in self.coords:
            for comp in F.comps(c):
                w += limbs(comp)
        return w + [int(self.flags[0]), int(self.flags[1])]


# ---------------------------------------------------------------- the three families
@functools.lru_cache(maxsize=None)
def _curve_points(g2):
    F = FIELDS[g2]
    rnd = random.Random(0x29C0 + g2)
    return [F.pmul(F.gen, rnd.randrange(1, bn.R)) for _ in range(6)]


def _nonzero_elem(F, rnd):
    while True:
        l = F.rand(rnd)
        if l != F.zero:
            return l


def xyzz_clothes(F, rnd, P, how=None, bounds=XYZZ_B):
    """The affine point P as (l^2 x + k1 q, l^3 y + k2 q, l^2 + k3 q, l^3 + k4 q), random l."""
    l = _nonzero_elem(F, rnd)
    l2 = F.mul(l, l); l3 = F.mul(l2, l)
    return [lift(F, rnd, v, H, how) for v, H in zip((F.mul(l2, P[0]), F.mul(l3, P[1]), l2, l3), bounds)]


def affine_clothes(F, rnd, P):
    return [lift(F, rnd, P[0], 2, "low"), lift(F, rnd, P[1], 2, "low")]


def _inf_xyzz(F):
    return [F.zero] * 4


class _Gen:
    """Record sources of one (group, op): each call of a source returns one record."""

    def __init__(self, g2, op):
        self.F, self.op = FIELDS[g2], op
        self.rnd = random.Random(0x29C0DE00 + 16 * g2 + op)
        self.pts = _curve_points(g2)
        self.n_special = 0

    def flags(self):
        return (self.rnd.randrange(2), self.rnd.randrange(2)) if self.op == 1 else (self.rnd.randrange(2), 0) if self.op == 0 else (0, 0)

    # -- coordinates at the bound limits (and random ones)
    def limits(self, p_edge=0.65):
        F, op, rnd = self.F, self.op, self.rnd
        k = self.n_special
        self.n_special += 1
        kinds = 5
        if k < 4 * kinds:     # every coordinate at the same limit at once, under every flag combination
            def at(H, nz):
                top, fl = max_value(H), H * Q // 2
                ev = edge_values(H, nz)
                v = (top, fl - 1, fl - 2, [e for e in ev if e & ((1 << 232) - 1) == (1 << 232) - 1][-1], [e for e in ev if e % Q == 1][-1])[k % kinds]
                return F.join(tuple(v for _ in F.comps(F.zero)))
            coords = [at(H, i in NONZERO[op]) for i, H in enumerate(IN_BOUNDS[op])]
            fl = ((k // kinds) & 1, (k // kinds) >> 1) if op in (0, 1) else (0, 0)
            return Record(coords, (fl[0], fl[1] if op == 1 else 0), "limits")
        coords = [pick_coord(F, rnd, H, i in NONZERO[op], p_edge) for i, H in enumerate(IN_BOUNDS[op])]
        return Record(coords, self.flags(), "limits" if p_edge else "random")

    def randoms(self):
        return self.limits(0.0)

    # -- the same x by construction, on coordinates at the limits: doubling (same=True) or cancellation
    def limits_same_x(self, same):
        F, op, rnd = self.F, self.op, self.rnd
        if op == 1:
            a = [pick_coord(F, rnd, 2, i == 1) for i in range(2)]
            na, spell = rnd.randrange(2), rnd.randrange(2)     # b = a, or b = -a under the other flag
            by = a[1] if not spell else lift(F, rnd, F.neg(decode(F, a[1])), 2, "low")
            nb = na ^ spell ^ (0 if same else 1)
            return Record(a + [a[0], by], (na, nb), "limits")
        if op == 0:
            q = [pick_coord(F, rnd, 2, i == 1) for i in range(2)]
            zz, zzz = pick_coord(F, rnd, HY, True), pick_coord(F, rnd, HY, True)
            neg_q = rnd.randrange(2)
            qy = decode(F, q[1])
            y = F.mul(qy if neg_q ^ same else F.neg(qy), decode(F, zzz))   # acc.Y = +-q.y ZZZ with the flag's sign: the same point, or its negative
            return Record([lift(F, rnd, F.mul(decode(F, q[0]), decode(F, zz)), HX), lift(F, rnd, y, HY), zz, zzz] + q, (neg_q, 0), "limits")
        # op 2: a = b in other clothes: (m^2 X, +-m^3 Y, m^2 ZZ, m^3 ZZZ)
        b = [pick_coord(F, rnd, H, i in (1, 2, 3)) for i, H in enumerate(XYZZ_B)]
        m = _nonzero_elem(F, rnd)
        m2 = F.mul(m, m); m3 = F.mul(m2, m)
        vb = [decode(F, c) for c in b]
        ya = F.mul(m3, vb[1])
        a = [lift(F, rnd, F.mul(m2, vb[0]), HX), lift(F, rnd, ya if same else F.neg(ya), HY), lift(F, rnd, F.mul(m2, vb[2]), HY), lift(F, rnd, F.mul(m3, vb[3]), HY)]
        return Record(a + b, (0, 0), "limits")

    # -- points of the curve in non-canonical clothes
    def curve(self, want):
        F, op, rnd = self.F, self.op, self.rnd
        P, S = rnd.sample(self.pts, 2)
        how = rnd.choice(("high", "high", None))
        mk = lambda coords, flags, expect: Record(coords, flags, "curve", expect, True)
        if op in (0, 1):
            if want == "inf":        # op 0 only: onto the empty accumulator
                n = rnd.randrange(2)
                return mk(_inf_xyzz(F) + affine_clothes(F, rnd, P), (n, 0), F.pneg(P) if n else P)
            na, nb = rnd.randrange(2), rnd.randrange(2)
            sP = F.pneg(P) if na else P                       # the first operand as it is meant
            other = {"general": S, "dbl": sP, "cancel": F.pneg(sP)}[want]   # the second, as it is meant
            written = F.pneg(other) if nb else other          # ... and as it is written under its flag
            if op == 1:
                return mk(affine_clothes(F, rnd, P) + affine_clothes(F, rnd, written), (na, nb), F.padd(sP, other))
            return mk(xyzz_clothes(F, rnd, sP, how) + affine_clothes(F, rnd, written), (nb, 0), F.padd(sP, other))
        if op == 2:
            if want == "inf":
                k = rnd.randrange(3)
                a = _inf_xyzz(F) if k != 1 else xyzz_clothes(F, rnd, P, how)
                b = _inf_xyzz(F) if k != 0 else xyzz_clothes(F, rnd, P, how)
                return mk(a + b, (0, 0), None if k == 2 else P)
            other = {"general": S, "dbl": P, "cancel": F.pneg(P)}[want]
            return mk(xyzz_clothes(F, rnd, P, how) + xyzz_clothes(F, rnd, other, rnd.choice(("high", None))), (0, 0), F.padd(P, other))
        if op == 3:
            return mk(_inf_xyzz(F), (0, 0), None) if want == "inf" else mk(xyzz_clothes(F, rnd, P, how), (0, 0), F.padd(P, P))
        if op == 4:
            return mk(affine_clothes(F, rnd, P), (0, 0), F.padd(P, P))
        if op == 5:
            l = _nonzero_elem(F, rnd)
            l2 = F.mul(l, l)
            return mk([lift(F, rnd, v, H, how) for v, H in zip((F.mul(l2, P[0]), F.mul(F.mul(l2, l), P[1]), l), (JX, JY, JZ))], (0, 0), F.padd(P, P))
        if want == "inf":            # op 6: infinity is ZZ = exact zeros, whatever the rest holds
            c = _inf_xyzz(F) if rnd.randrange(2) else [pick_coord(F, rnd, HX, False), pick_coord(F, rnd, HY, True), F.zero, pick_coord(F, rnd, HY, False)]
            return mk(c, (0, 0), None)
        return mk(xyzz_clothes(F, rnd, P, how), (0, 0), P)

    # -- Fq2: an x difference (t, +-t), t != 0: the real part of its square vanishes, the square does not
    def zero_test(self):
        F, op, rnd = self.F, self.op, self.rnd
        assert F.g2 and op in (0, 1, 2)
        t = rnd.choice((1, Q - 1, RADIX % Q, rnd.randrange(1, Q)))          # as the limbs hold it (x 2^261), so 1 and q - 1 are the raw values
        d = decode(F, (t, t if rnd.randrange(2) else Q - t))
        if op == 1:
            a = [pick_coord(F, rnd, 2, i == 1, 0.3) for i in range(2)]
            return Record(a + [lift(F, rnd, F.add(decode(F, a[0]), d), 2, "low"), pick_coord(F, rnd, 2, True, 0.3)], self.flags(), "zerotest")
        if op == 0:                                                        # ZZ = 1: q.x ZZ - X = q.x - X
            q = [pick_coord(F, rnd, 2, i == 1, 0.3) for i in range(2)]
            x = lift(F, rnd, F.sub(decode(F, q[0]), d), HX)
            return Record([x, pick_coord(F, rnd, HY, True, 0.3), lift(F, rnd, F.one, HY), pick_coord(F, rnd, HY, True, 0.3)] + q, self.flags(), "zerotest")
        a = [pick_coord(F, rnd, H, i in (1, 2, 3), 0.3) for i, H in enumerate(XYZZ_B)]
        b = [pick_coord(F, rnd, H, i in (1, 2, 3), 0.3) for i, H in enumerate(XYZZ_B)]
        if rnd.randrange(2):
            a[2] = lift(F, rnd, F.one, HY); b[2] = lift(F, rnd, F.one, HY)
        va, vb = [decode(F, c) for c in a], [decode(F, c) for c in b]
        b[0] = lift(F, rnd, F.mul(F.add(F.mul(va[0], vb[2]), d), F.inv(va[2])), HX)   # X2 ZZ1 - X1 ZZ2 = d
        return Record(a + b, (0, 0), "zerotest")


def x_difference(F, op, rec):
    """P of the addition `op` on this record (the difference of the x coordinates brought to one denominator)."""
    v = [decode(F, c) for c in rec.coords]
    if op == 0:
        return F.sub(F.mul(v[4], v[2]), v[0])
    if op == 1:
        return F.sub(v[2], v[0])
    return F.sub(F.mul(v[4], v[2]), F.mul(v[0], v[6]))


class Cases:
    """The records of one (group, op) in their final order, their words, and the model's verdict on each."""

    def __init__(self, g2, op):
        self.g2, self.op, self.F = g2, op, FIELDS[g2]
        F, gen = self.F, _Gen(g2, op)
        rnd = gen.rnd
        branches = BRANCHES[op]
        rare = [b for b in branches if b != "general"]
        uniform = ["general", "dbl" if "dbl" in branches else "general"]
        per_block, per_tail = 8, 4
        tail = N_RECORDS - 64 * (N_MIXED + 2)
        need = {b: N_MIXED * per_block + per_tail + 64 * uniform.count(b) for b in rare}
        need["general"] = N_RECORDS - sum(need.values())
        pools = {b: [] for b in branches}
        zero_ok = bool(g2) and op in (0, 1, 2)
        sources = {"general": [gen.limits, gen.limits, lambda: gen.curve("general"), gen.randoms] + ([gen.zero_test] if zero_ok else []),
                   "dbl": [lambda: gen.curve("dbl"), lambda: gen.limits_same_x(True)],
                   "cancel": [lambda: gen.curve("cancel"), lambda: gen.limits_same_x(False)],
                   "inf": [lambda: gen.curve("inf")]}
        for b in branches:
            k = 0
            while len(pools[b]) < need[b]:
                rec = sources[b][k % len(sources[b])]()
                k += 1
                res, br = model(F, op, rec.coords, rec.flags)
                if len(pools[br]) < need[br]:          # a record lands in the pool of the branch the MODEL gives it
                    pools[br].append((rec, res, br))
            rnd.shuffle(pools[b])
        order = []
        for blk in range(N_MIXED):
            block = [pools[b].pop() for b in rare for _ in range(per_block)]
            block += [pools["general"].pop() for _ in range(64 - len(block))]
            rnd.shuffle(block)
            order += block
        for b in uniform:
            order += [pools[b].pop() for _ in range(64)]
        block = [pools[b].pop() for b in rare for _ in range(per_tail)]
        block += [pools["general"].pop() for _ in range(tail - len(block))]
        rnd.shuffle(block)
        order += block
        assert all(not p for p in pools.values()) and len(order) == N_RECORDS
        self.recs = [o[0] for o in order]
        self.want = [o[1] for o in order]
        self.branch = [o[2] for o in order]
        self._words = None
        self._self_check(uniform, zero_ok)

    def _self_check(self, uniform, zero_ok):
        """What the order promises, from the model's own verdicts."""
        F, op, br = self.F, self.op, self.branch
        for b in BRANCHES[op]:
            assert br.count(b) >= 64, (op, b)
        for blk in range(N_MIXED):
            assert set(br[64 * blk:64 * blk + 64]) == set(BRANCHES[op]), (op, blk)
        for k, b in enumerate(uniform):
            assert set(br[64 * (N_MIXED + k):64 * (N_MIXED + k + 1)]) == {b}, (op, b)
        assert set(br[64 * (N_MIXED + 2):]) == set(BRANCHES[op])
        fam = [r.family for r in self.recs]
        assert fam.count("limits") >= 256 and fam.count("curve") >= 128 and fam.count("random") >= 64
        for rec in self.recs:
            for i, (c, H) in enumerate(zip(rec.coords, IN_BOUNDS[op])):
                comps = F.comps(c)
                assert all(0 <= v <= max_value(H) for v in comps), (op, i)
                zz = 2 if i < 4 and op in (0, 2, 3, 6) else 6 if op == 2 else None    # the ZZ of the point this coordinate belongs to
                if i in NONZERO[op] and not (zz is not None and is_zero_raw(F, rec.coords[zz])):   # infinity is exact zeros
                    assert any(v % Q for v in comps), (op, i, rec.family)
        if zero_ok:
            zt = [i for i, f in enumerate(fam) if f == "zerotest"]
            assert len(zt) >= 64
            for i in zt:
                p = x_difference(F, op, self.recs[i])
                pp = F.mul(p, p)
                assert pp[0] == 0 and pp[1] != 0 and br[i] == "general", (op, i)

    def words(self):
        """The records as one ctypes array of uint32, made once."""
        if self._words is None:
            import ctypes
            flat = [w for r in self.recs for w in r.words(self.F)]
            self._words = (ctypes.c_uint32 * len(flat))(*flat)
        return self._words


@functools.lru_cache(maxsize=None)
def cases(g2, op):
    return Cases(g2, op)


# ---------------------------------------------------------------- what every result has to satisfy
def words_per(g2, op):
    nl = 18 if g2 else 9
    n_in = len(IN_BOUNDS[op])
    return n_in * nl + 2, 3 * nl if op == 5 else 4 * nl + (4 * (16 if g2 else 8) if op == 6 else 0)


def _coords_from_limbs(F, w, n):
    """n coordinates from 9 / 18 limbs each: (raw values, every limb in range)."""
    nl = 18 if F.g2 else 9
    vals, ok = [], True
    for i in range(n):
        comps = []
        for j in range(0, nl, 9):
            l = w[i * nl + j:i * nl + j + 9]
            ok = ok and all(x < (1 << 29) for x in l[:8]) and l[8] < (1 << 28)
            comps.append(limbs_value(l))
        vals.append(F.join(tuple(comps)))
    return vals, ok


def check_results(cs, out, inf, build):
    """Every record of `cs` against the model: value mod q, bound of the type, limb ranges, infinity = exact zeros + flag.  Returns
    the number of records checked (all of them); an assertion names the build, group, operation, record, family and branch."""
    F, op = cs.F, cs.op
    ow = words_per(cs.g2, op)[1]
    assert len(out) == ow * N_RECORDS and len(inf) == N_RECORDS
    n_out = len(OUT_BOUNDS[op])
    for i, (rec, want, br) in enumerate(zip(cs.recs, cs.want, cs.branch)):
        tag = "%s %s %s record %d (%s, %s)" % (build, "G2" if cs.g2 else "G1", OP_NAMES[op], i, rec.family, br)
        w = out[i * ow:(i + 1) * ow]
        if op == 6:
            nw = 16 if cs.g2 else 8
            packed = [F.join(tuple(sum(int(x) << (32 * k) for k, x in enumerate(w[c * nw + j:c * nw + j + 8])) for j in range(0, nw, 8))) for c in range(4)]
            back, ok = _coords_from_limbs(F, w[4 * nw:], 4)
            assert ok, tag + ": limb out of range after unpack_xyzz"
            assert back == packed, tag + ": unpack_xyzz does not give back the packed words"
            assert (want is None) == (inf[i] == 1) == (not any(w)), tag + ": infinity is not exact zeros with the flag"
            if want is not None:
                assert all(c < 2 * Q for v in packed for c in F.comps(v)), tag + ": a packed word string is not below 2 q"
                assert tuple(decode(F, v) for v in packed) == want, tag + ": value changed mod q"
            continue
        vals, ok = _coords_from_limbs(F, w, n_out)
        assert ok, tag + ": limb out of range"
        assert (want is None) == (inf[i] == 1) == (not any(w)), tag + ": infinity is not exact zeros with the flag"
        if want is None:
            continue
        for name, v, H, e in zip(("X", "Y", "Z") if op == 5 else ("X", "Y", "ZZ", "ZZZ"), vals, OUT_BOUNDS[op], want):
            assert all(2 * c < H * Q for c in F.comps(v)), tag + ": %s is not below %d half moduli" % (name, H)
            assert decode(F, v) == e, tag + ": %s differs from the integer model" % name
        if rec.has_expect:
            assert to_affine(F, tuple(decode(F, v) for v in vals)) == rec.expect, tag + ": not the oracle's point"
    return N_RECORDS
