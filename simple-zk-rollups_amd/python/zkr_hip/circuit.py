"""A small circuit builder: one description of a circuit -> its constraints (r1cs_bin, as ProvingKey.setup_r1cs and
ConstraintSystem.load take them) AND its witness program (wprog_bin, include/zkr.h, as WitnessProgram takes it).  A user circuit
then runs witness -> check -> prove -> verify on the GPU without circom and without a line of device code.

Values are linear combinations (LC) of signals, tracked symbolically: adding, subtracting and scaling cost no constraint and no
signal.  A multiplication defines a signal and a constraint (`s <== a * b + c` in circom's words).  On the program side every signal
has a wire, and a linear combination is turned into instructions only where a product, a hint or an assertion needs its value.

Signal order is snarkjs's: one, outputs, public inputs, private inputs, internals; n_public = outputs + public inputs.  The
program's inputs are the public inputs followed by the private inputs, each in declaration order (Circuit.input_names).

    c = Circuit()
    out = c.output("hash")
    x, y = c.public_input("x"), c.private_input("y")
    c.assign(out, gadgets.multi_hash(c, [x, y]))
    key, vk = ProvingKey.setup_r1cs(c.r1cs()); prog = WitnessProgram(c.program(), statements=c.statements)
"""
import struct

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
WPROG_MAGIC, WPROG_VERSION = 0x50574B5A, 1
OP_CONST, OP_ADD, OP_SUB, OP_MUL, OP_INV0, OP_BIT, OP_ASSERT_ZERO = 1, 2, 3, 4, 5, 6, 7
MIMC_ROUNDS = 220   # hasher.circom:8
BJ_A, BJ_D = 168700, 168696   # BabyJub: a x^2 + y^2 = 1 + d x^2 y^2


class Signal:
    __slots__ = ("kind", "name", "uid", "wire")

    def __init__(self, kind, name, uid):
        self.kind, self.name, self.uid, self.wire = kind, name, uid, None   # wire: self for an input, an instruction's ordinal otherwise

    def __repr__(self):
        return "<%s %s>" % (self.kind, self.name)


class LC:
    """sum of coefficient x signal, coefficients mod r; immutable.  Integers mix in as multiples of the signal `one`."""
    __slots__ = ("c", "terms")

    def __init__(self, circuit, terms=None):
        self.c = circuit
        self.terms = {s: v % R for s, v in (terms or {}).items() if v % R}

    def _lift(self, o):
        if isinstance(o, LC):
            if o.c is not self.c:
                raise ValueError("linear combinations of two circuits")
            return o
        return LC(self.c, {self.c.one: int(o)})

    def __add__(self, o):
        o = self._lift(o)
        t = dict(self.terms)
        for s, v in o.terms.items():
            t[s] = t.get(s, 0) + v
        return LC(self.c, t)

    __radd__ = __add__

    def __neg__(self):
        return LC(self.c, {s: -v for s, v in self.terms.items()})

    def __sub__(self, o):
        return self + (-self._lift(o))

    def __rsub__(self, o):
        return self._lift(o) - self

    def __mul__(self, k):
        if isinstance(k, LC):
            raise TypeError("a product of two linear combinations is a constraint: use Circuit.mul")
        return LC(self.c, {s: v * int(k) for s, v in self.terms.items()})

    __rmul__ = __mul__

    def key(self):
        return tuple(sorted((s.uid, v) for s, v in self.terms.items()))


class Hint:
    """A value that lives on a wire of the program and is NO signal: what circom computes with `<--` before it names the result.
    Lifted from a linear combination (Circuit.hint), it combines with +, -, * and inv() -- ADD, SUB, MUL and INV0 on the program
    side, nothing on the constraint side -- and Circuit.witness makes it a signal.  Immutable."""
    __slots__ = ("c", "wire")

    def __init__(self, circuit, wire):
        self.c, self.wire = circuit, wire

    def _lift(self, o):
        if isinstance(o, Hint):
            if o.c is not self.c:
                raise ValueError("hint values of two circuits")
            return o
        return self.c.hint(o)

    def _op(self, op, a, b):
        return Hint(self.c, self.c._emit(op, a.wire, b.wire))

    def __add__(self, o):
        return self._op(OP_ADD, self, self._lift(o))

    def __radd__(self, o):
        return self._op(OP_ADD, self._lift(o), self)

    def __sub__(self, o):
        return self._op(OP_SUB, self, self._lift(o))

    def __rsub__(self, o):
        return self._op(OP_SUB, self._lift(o), self)

    def __mul__(self, o):
        return self._op(OP_MUL, self, self._lift(o))

    def __rmul__(self, o):
        return self._op(OP_MUL, self._lift(o), self)

    def inv(self):
        """0 for 0, the inverse otherwise (INV0)"""
        return Hint(self.c, self.c._emit(OP_INV0, self.wire))


class Circuit:
    def __init__(self):
        self._uid = 0
        self.one = self._signal("one", "one")
        self.one.wire = self.one
        self.outputs, self.publics, self.privates, self.internals = [], [], [], []
        self.constraints = []    # (A, B, C) linear combinations: A * B = C
        self.statements = []     # statement id -> text (ASSERT_ZERO's second operand)
        self._consts, self._const_index = [], {}
        self._instr = []         # (op, a, b): operands are wires (a Signal for wire 0 and the inputs, else the ordinal of the defining instruction) or plain numbers
        self._n_defined = 0
        self._const_wire, self._term_wire, self._lc_wire = {}, {}, {}

    # ---- declarations
    def _signal(self, kind, name):
        s = Signal(kind, name, self._uid)
        self._uid += 1
        return s

    def const(self, v=0):
        return LC(self, {self.one: int(v)})

    def output(self, name=None):
        s = self._signal("output", name or "out%d" % len(self.outputs))
        self.outputs.append(s)
        return LC(self, {s: 1})

    def public_input(self, name=None):
        s = self._signal("public", name or "pub%d" % len(self.publics))
        s.wire = s
        self.publics.append(s)
        return LC(self, {s: 1})

    def private_input(self, name=None):
        s = self._signal("private", name or "priv%d" % len(self.privates))
        s.wire = s
        self.privates.append(s)
        return LC(self, {s: 1})

    @property
    def input_names(self):
        return [s.name for s in self.publics + self.privates]

    @property
    def n_inputs(self):
        return len(self.publics) + len(self.privates)

    @property
    def n_public(self):
        return len(self.outputs) + len(self.publics)

    @property
    def n_vars(self):
        return 1 + len(self.outputs) + len(self.publics) + len(self.privates) + len(self.internals)

    def signals(self):
        return [self.one] + self.outputs + self.publics + self.privates + self.internals

    # ---- the program side
    def _emit(self, op, a=0, b=0):
        self._instr.append((op, a, b))
        if op == OP_ASSERT_ZERO:
            return None
        self._n_defined += 1
        return self._n_defined - 1

    def _constant(self, v):
        """wire holding the constant v"""
        v %= R
        if v == 1:
            return self.one
        if v not in self._const_wire:
            if v not in self._const_index:
                self._const_index[v] = len(self._consts)
                self._consts.append(v)
            self._const_wire[v] = self._emit(OP_CONST, self._const_index[v])
        return self._const_wire[v]

    def _wire(self, lc):
        """the wire that holds the value of a linear combination: its instructions are emitted once"""
        lc = lc if isinstance(lc, LC) else self.const(lc)
        k = lc.key()
        if k in self._lc_wire:
            return self._lc_wire[k]
        plus, minus = [], []
        for s, v in sorted(lc.terms.items(), key=lambda t: t[0].uid):
            if s is not self.one and s.wire is None:
                raise ValueError("output %s is used before Circuit.assign gives it a value" % s.name)
            if s is self.one:
                plus.append(self._constant(v))
            elif v == 1:
                plus.append(s.wire)
            elif v == R - 1:
                minus.append(s.wire)
            else:
                if (s.uid, v) not in self._term_wire:
                    self._term_wire[(s.uid, v)] = self._emit(OP_MUL, self._constant(v), s.wire)
                plus.append(self._term_wire[(s.uid, v)])
        acc = plus[0] if plus else self._constant(0)
        for w in plus[1:]:
            acc = self._emit(OP_ADD, acc, w)
        for w in minus:
            acc = self._emit(OP_SUB, acc, w)
        self._lc_wire[k] = acc
        return acc

    def _internal(self, wire, name):
        s = self._signal("internal", name or "s%d" % len(self.internals))
        s.wire = wire
        self.internals.append(s)
        return LC(self, {s: 1})

    # ---- what a circuit is made of
    def mul(self, a, b, add=None, name=None):
        """a new signal s = a * b + add, with the constraint a * b = s - add"""
        a, b = self.const(0) + a, self.const(0) + b
        w = self._emit(OP_MUL, self._wire(a), self._wire(b))
        add = None if add is None else self.const(0) + add
        if add is not None and add.terms:
            w = self._emit(OP_ADD, w, self._wire(add))
        s = self._internal(w, name)
        self.constraints.append((a, b, s - add if add is not None else s))
        return s

    def hint_bit(self, a, i, name=None):
        """a new signal: bit i of the canonical value of a.  No constraint: the caller adds them (gadgets.num2bits)."""
        if not 0 <= i < 254:
            raise ValueError("bit index %d is not below 254" % i)
        return self._internal(self._emit(OP_BIT, self._wire(self.const(0) + a), i), name)

    def hint_inv0(self, a, name=None):
        """a new signal: 0 for 0, the inverse of a otherwise.  No constraint: the caller adds them (gadgets.is_zero)."""
        return self._internal(self._emit(OP_INV0, self._wire(self.const(0) + a)), name)

    def hint(self, lc):
        """the value of a linear combination (or a number) as a Hint: computed by the program, unknown to the constraints"""
        if isinstance(lc, Hint):
            return lc
        return Hint(self, self._wire(self.const(0) + lc))

    def witness(self, value, name=None):
        """a new signal that takes a Hint's value, with no constraint (circom's `<--`): the caller adds them"""
        if not isinstance(value, Hint) or value.c is not self:
            raise ValueError("witness takes a hint value of this circuit")
        return self._internal(value.wire, name)

    def _statement(self, text):
        self.statements.append(text)
        return len(self.statements) - 1

    def constrain(self, a, b, c, text=None):
        """the constraint a * b = c.  With a text the program checks it too (a statement that an instance's inputs can violate);
        without one it is taken to hold by construction."""
        a, b, c = self.const(0) + a, self.const(0) + b, self.const(0) + c
        self.constraints.append((a, b, c))
        if text is not None:
            w = self._emit(OP_MUL, self._wire(a), self._wire(b))
            if c.terms:
                w = self._emit(OP_SUB, w, self._wire(c))
            self._emit(OP_ASSERT_ZERO, w, self._statement(text))

    def assert_zero(self, lc, text):
        """the constraint lc * 1 = 0 and the program's check of it, reported with `text`"""
        lc = self.const(0) + lc
        self.constraints.append((lc, self.const(1), self.const(0)))
        self._emit(OP_ASSERT_ZERO, self._wire(lc), self._statement(text))

    def assign(self, out, lc):
        """out <== lc for a declared output: the constraint lc * 1 = out"""
        (s, v), = out.terms.items()
        if s.kind != "output" or v != 1 or s.wire is not None:
            raise ValueError("assign takes an output that has no value yet")
        lc = self.const(0) + lc
        s.wire = self._wire(lc)
        self.constraints.append((lc, self.const(1), out))

    # ---- the two files
    def r1cs(self) -> bytes:
        """r1cs_bin (zkr.h, zkr_setup_r1cs)"""
        index = {s: k for k, s in enumerate(self.signals())}
        out = [struct.pack("<III", self.n_vars, self.n_public, len(self.constraints))]
        for abc in self.constraints:
            for lc in abc:
                terms = sorted((index[s], v) for s, v in lc.terms.items())
                out.append(struct.pack("<I", len(terms)))
                out.extend(struct.pack("<I", k) + v.to_bytes(32, "little") for k, v in terms)
        return b"".join(out)

    def program(self) -> bytes:
        """wprog_bin (zkr.h, zkr_wprog_load)"""
        for s in self.outputs:
            if s.wire is None:
                raise ValueError("output %s has no value: Circuit.assign" % s.name)
        inputs = {s: 1 + k for k, s in enumerate(self.publics + self.privates)}
        first = 1 + len(inputs)

        def wire(x):
            return 0 if x is self.one else inputs[x] if isinstance(x, Signal) else first + x

        out = [struct.pack("<8I", WPROG_MAGIC, WPROG_VERSION, len(inputs), len(self._consts), len(self._instr), self.n_vars, self.n_public, len(self.statements))]
        out.extend(v.to_bytes(32, "little") for v in self._consts)
        for op, a, b in self._instr:
            if op == OP_CONST:
                out.append(struct.pack("<4I", op, a, 0, 0))
            elif op in (OP_INV0,):
                out.append(struct.pack("<4I", op, wire(a), 0, 0))
            elif op in (OP_BIT, OP_ASSERT_ZERO):
                out.append(struct.pack("<4I", op, wire(a), b, 0))
            else:
                out.append(struct.pack("<4I", op, wire(a), wire(b), 0))
        out.append(struct.pack("<%dI" % self.n_vars, *[wire(s.wire) for s in self.signals()]))
        return b"".join(out)

    def counts(self):
        """instructions by opcode name, for the paper counts of DESIGN.md 9l"""
        names = {OP_CONST: "CONST", OP_ADD: "ADD", OP_SUB: "SUB", OP_MUL: "MUL", OP_INV0: "INV0", OP_BIT: "BIT", OP_ASSERT_ZERO: "ASSERT_ZERO"}
        out = {}
        for op, _, _ in self._instr:
            out[names[op]] = out.get(names[op], 0) + 1
        return out


_mimc = None


def _mimc_constants():
    global _mimc
    if _mimc is None:
        from .binding import mimcsponge_round_constants
        _mimc = mimcsponge_round_constants()
    return _mimc


class gadgets:
    """Compositions over Circuit: what the engine leaves to the front end."""

    @staticmethod
    def num2bits(c, x, n, text=None):
        """n bits of x, least significant first: each boolean (b (b - 1) = 0), together recomposing x (asserted: it fails for x >= 2^n)"""
        bits = [c.hint_bit(x, i) for i in range(n)]
        acc = c.const(0)
        for i, b in enumerate(bits):
            c.constrain(b, b - 1, 0)
            acc = acc + b * (1 << i)
        c.assert_zero(acc - x, text or "value fits %d bits" % n)
        return bits

    @staticmethod
    def is_zero(c, x):
        """1 when x is 0, else 0 (circomlib IsZero: out = -x inv + 1, x out = 0)"""
        inv = c.hint_inv0(x)
        out = c.mul(x, -inv, add=1)
        c.constrain(x, out, 0)
        return out

    @staticmethod
    def select(c, s, a, b):
        """a when s is 1, b when s is 0; s must be constrained boolean by the caller"""
        return c.mul(s, (c.const(0) + a) - b, add=b)

    @staticmethod
    def mimc_feistel(c, xl, xr, k=0):
        """circomlib MiMCFeistel(220): three constraints a round (t^2, t^4, t^4 t + xR)"""
        cts = _mimc_constants()
        xl, xr = c.const(0) + xl, c.const(0) + xr
        for i in range(MIMC_ROUNDS):
            t = xl + k + cts[i]
            t2 = c.mul(t, t)
            t4 = c.mul(t2, t2)
            nxt = c.mul(t4, t, add=xr)
            if i < MIMC_ROUNDS - 1:
                xl, xr = nxt, xl
            else:
                xr = nxt
        return xl, xr

    @staticmethod
    def multi_hash(c, ins, key=0):
        """MiMCSponge(len(ins), 220, 1) (hasher.circom:3-16): absorb one input a permutation, one output"""
        r, cap = c.const(0), c.const(0)
        for x in ins:
            r, cap = gadgets.mimc_feistel(c, r + x, cap, key)
        return r

    @staticmethod
    def hash_left_right(c, left, right):
        return gadgets.multi_hash(c, [left, right])   # hasher.circom:18-30

    @staticmethod
    def merkle_root(c, leaf, path_elements, path_index_bits):
        """MerkleTreeRootConstructor (merkletree.circom:33-66): per level the index is asserted boolean, (left, right) = (in, element)
        for index 0 and (element, in) for 1 -- two products instead of PathSelector's four -- and hashed"""
        cur = c.const(0) + leaf
        for lvl, (pe, idx) in enumerate(zip(path_elements, path_index_bits)):
            c.constrain(idx, 1 - idx, 0, text="path index %d is 0 or 1" % lvl)
            left = c.mul(idx, pe - cur, add=cur)
            right = c.mul(idx, cur - pe, add=pe)
            cur = gadgets.hash_left_right(c, left, right)
        return cur

    @staticmethod
    def leaf_exists(c, leaf, path_elements, path_index_bits, root):
        """MerkleTreeLeafExists (merkletree.circom:68-84)"""
        c.assert_zero(root - gadgets.merkle_root(c, leaf, path_elements, path_index_bits), "the leaf is in the tree with this root")


    # ---- BabyJub (circomlib babyjub.circom, escalarmulany.circom)
    @staticmethod
    def babyjub_check(c, p, text):
        """BabyCheck: a x^2 + y^2 = 1 + d x^2 y^2, a statement the program checks and reports with `text`"""
        x, y = p
        x2, y2 = c.mul(x, x), c.mul(y, y)
        c.constrain(x2 * BJ_D, y2, x2 * BJ_A + y2 - 1, text=text)

    @staticmethod
    def babyjub_add(c, p, q, known=None):
        """BabyAdd's six constraints: beta = x1 y2, gamma = y1 x2, delta = (-a x1 + y1)(x2 + y2), tau = beta gamma,
        (1 + d tau) x3 = beta + gamma, (1 - d tau) y3 = delta + a beta - gamma.  The law is complete on the curve: no exceptional
        cases.  x3 and y3 are values the program computes: `known` = their Hints where the caller has them already (a chain that
        inverts once for all its points); otherwise one INV0 here for the two denominators."""
        (x1, y1), (x2, y2) = p, q
        beta, gamma = c.mul(x1, y2), c.mul(y1, x2)
        delta = c.mul(y1 - (c.const(0) + x1) * BJ_A, (c.const(0) + x2) + y2)
        tau = c.mul(beta, gamma)
        dx, dy = tau * BJ_D + 1, 1 - tau * BJ_D
        nx, ny = beta + gamma, delta + beta * BJ_A - gamma
        if known is None:
            hx, hy = c.hint(dx), c.hint(dy)
            i = (hx * hy).inv()
            known = (c.hint(nx) * (i * hy), c.hint(ny) * (i * hx))
        x3, y3 = c.witness(known[0]), c.witness(known[1])
        c.constrain(dx, x3, nx)
        c.constrain(dy, y3, ny)
        return x3, y3

    @staticmethod
    def babyjub_dbl(c, p, known=None):
        return gadgets.babyjub_add(c, p, p, known)

    @staticmethod
    def _proj_add(p, q):
        """add-2008-bbjlp on hint values (X : Y : Z)"""
        (x1, y1, z1), (x2, y2, z2) = p, q
        a = z1 * z2
        b, cc, d = a * a, x1 * x2, y1 * y2
        e = (cc * d) * BJ_D
        f, g = b - e, b + e
        return (a * f) * ((x1 + y1) * (x2 + y2) - cc - d), (a * g) * (d - cc * BJ_A), f * g

    @staticmethod
    def _proj_dbl(p):
        """dbl-2008-bbjlp on hint values"""
        x, y, z = p
        s = x + y
        b, cc, d = s * s, x * x, y * y
        e = cc * BJ_A
        f, h = e + d, z * z
        j = f - (h + h)
        return (b - cc - d) * j, f * (e - d), f * j

    @staticmethod
    def _affine_all(c, pts):
        """affine Hints of projective hint points with ONE inversion (Montgomery's trick): prefix products, INV0, the walk back"""
        prefix, run = [], c.hint(1)
        for _, _, z in pts:
            prefix.append(run)
            run = run * z
        ia, out = run.inv(), [None] * len(pts)
        for k in range(len(pts) - 1, -1, -1):
            x, y, z = pts[k]
            zi = ia * prefix[k]
            ia = ia * z
            out[k] = (x * zi, y * zi)
        return out

    @staticmethod
    def escalar_mul_any(c, bits, p, text="the point is on the curve"):
        """e * p for e = sum of bits[i] 2^i (bits: boolean signals, least significant first) and any point p of the curve:
        babyjub_check on p first (an off-curve p is a reported statement), then double-and-add -- per bit a doubling of 2^i p, an
        addition to the running sum and an arithmetic select of the two coordinates, 14 constraints.  The witness side never
        divides per step: it walks the same points in projective coordinates on hint values and inverts all their Z at once.  On
        the curve no Z is 0; off it the instance has failed its statement and is zeroed whatever the hints hold."""
        p = (c.const(0) + p[0], c.const(0) + p[1])
        gadgets.babyjub_check(c, p, text)
        n = len(bits)
        # the program's own walk: Q_i = 2^i p, S_i = A_{i-1} + Q_i, A_i = bits[i] ? S_i : A_{i-1}
        one = c.hint(1)
        q = (c.hint(p[0]), c.hint(p[1]), one)
        b0 = c.hint(bits[0])
        acc = (b0 * q[0], b0 * (q[1] - 1) + 1, one)
        doubles, sums = [], []
        for i in range(1, n):
            q = gadgets._proj_dbl(q)
            s = gadgets._proj_add(acc, q)
            b = c.hint(bits[i])
            acc = tuple(b * (sv - av) + av for sv, av in zip(s, acc))
            doubles.append(q)
            sums.append(s)
        aff = gadgets._affine_all(c, doubles + sums)
        # the constraints, over signals that take those values
        qa = p
        ax, ay = c.mul(bits[0], p[0]), c.mul(bits[0], p[1] - 1, add=1)
        for i in range(1, n):
            qa = gadgets.babyjub_dbl(c, qa, known=aff[i - 1])
            sx, sy = gadgets.babyjub_add(c, (ax, ay), qa, known=aff[n - 1 + i - 1])
            ax, ay = gadgets.select(c, bits[i], sx, ax), gadgets.select(c, bits[i], sy, ay)
        return ax, ay


# ---- the reference's wrapper circuits (prover/__tests__/circuits/*_test.circom), as this builder states them
def Hasher(length):
    """inputs in[length], key; output hash"""
    c = Circuit()
    out = c.output("hash")
    ins = [c.public_input("in[%d]" % i) for i in range(length)]
    key = c.public_input("key")
    c.assign(out, gadgets.multi_hash(c, ins, key))
    return c


def HashLeftRight():
    c = Circuit()
    out = c.output("hash")
    left, right = c.public_input("left"), c.public_input("right")
    c.assign(out, gadgets.hash_left_right(c, left, right))
    return c


def MerkleTreeRootConstructor(depth):
    """inputs leaf | pathElements[depth], pathIndexes[depth] (private); output root"""
    c = Circuit()
    out = c.output("root")
    leaf = c.public_input("leaf")
    pes = [c.private_input("pathElements[%d]" % i) for i in range(depth)]
    idx = [c.private_input("pathIndexes[%d]" % i) for i in range(depth)]
    c.assign(out, gadgets.merkle_root(c, leaf, pes, idx))
    return c


def MerkleTreeLeafExists(depth):
    """inputs leaf, root | pathElements[depth], pathIndexes[depth] (private); no output"""
    c = Circuit()
    leaf, root = c.public_input("leaf"), c.public_input("root")
    pes = [c.private_input("pathElements[%d]" % i) for i in range(depth)]
    idx = [c.private_input("pathIndexes[%d]" % i) for i in range(depth)]
    gadgets.leaf_exists(c, leaf, pes, idx, root)
    return c


def Ecdh():
    """prover/circuits/ecdh.circom:6-27: inputs publicKey[0..1] | privateKey (private, the FORMATTED key); output sharedKey, the x
    coordinate of privateKey * publicKey"""
    c = Circuit()
    out = c.output("sharedKey")
    pub = [c.public_input("publicKey[%d]" % i) for i in range(2)]
    priv = c.private_input("privateKey")
    bits = gadgets.num2bits(c, priv, 253, "private key fits 253 bits")
    x, _ = gadgets.escalar_mul_any(c, bits, pub, "public key is on the curve")
    c.assign(out, x)
    return c
