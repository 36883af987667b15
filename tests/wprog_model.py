"""An interpreter of wprog_bin in Python integers, written from the format's description in include/zkr.h and from nothing else, and
a small generator of random programs for the engine tests (tests/test_wprog_cpu.py on the host twin, tests/test_gpu_wprog.py on
the device).  The interpreter does not validate: it is handed programs the generator made."""
import random
import struct

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MAGIC, VERSION = 0x50574B5A, 1
CONST, ADD, SUB, MUL, INV0, BIT, ASSERT_ZERO = 1, 2, 3, 4, 5, 6, 7
HEADER = 32


def encode(n_inputs, consts, instrs, sigmap, n_public, n_statements, magic=MAGIC, version=VERSION):
    """header | constants | instructions (op, a, b, c) | signal map"""
    out = [struct.pack("<8I", magic, version, n_inputs, len(consts), len(instrs), len(sigmap), n_public, n_statements)]
    out += [int(v).to_bytes(32, "little") for v in consts]
    out += [struct.pack("<4I", *ins) for ins in instrs]
    out.append(struct.pack("<%dI" % len(sigmap), *sigmap))
    return b"".join(out)


def decode(blob):
    magic, version, n_inputs, n_consts, n_instr, n_vars, n_public, n_statements = struct.unpack_from("<8I", blob, 0)
    assert magic == MAGIC and version == VERSION
    off = HEADER
    consts = [int.from_bytes(blob[off + 32 * k:off + 32 * k + 32], "little") for k in range(n_consts)]
    off += 32 * n_consts
    instrs = [struct.unpack_from("<4I", blob, off + 16 * k) for k in range(n_instr)]
    off += 16 * n_instr
    sigmap = list(struct.unpack_from("<%dI" % n_vars, blob, off))
    assert off + 4 * n_vars == len(blob)
    return dict(n_inputs=n_inputs, consts=consts, instrs=instrs, map=sigmap, n_public=n_public, n_statements=n_statements)


def run(blob, inputs):
    """-> (code, statement, wires, witness): code 0 ok / 1 an input is not below r (statement = the first such input; wires and
    witness all zero) / 2 an assertion failed (statement of the FIRST failing one in program order; every wire is still computed,
    the witness is all zero)."""
    p = decode(blob)
    n_wires = 1 + p["n_inputs"] + sum(1 for ins in p["instrs"] if ins[0] != ASSERT_ZERO)
    assert len(inputs) == p["n_inputs"]
    for i, v in enumerate(inputs):
        if v >= R:
            return 1, i, [0] * n_wires, [0] * len(p["map"])
    w = [1] + [int(v) for v in inputs]
    code, stmt = 0, 0
    for op, a, b, _ in p["instrs"]:
        if op == CONST:
            w.append(p["consts"][a])
        elif op == ADD:
            w.append((w[a] + w[b]) % R)
        elif op == SUB:
            w.append((w[a] - w[b]) % R)
        elif op == MUL:
            w.append(w[a] * w[b] % R)
        elif op == INV0:
            w.append(pow(w[a], R - 2, R))
        elif op == BIT:
            w.append((w[a] >> b) & 1)
        elif op == ASSERT_ZERO:
            if w[a] != 0 and code == 0:
                code, stmt = 2, b
        else:
            raise ValueError(op)
    assert len(w) == n_wires
    return code, stmt, w, [w[k] if code == 0 else 0 for k in p["map"]]


EDGE_VALUES = (0, 1, 2, R - 1, R - 2)


def random_inputs(rng, n_inputs):
    return [rng.choice(EDGE_VALUES) if rng.random() < 0.5 else rng.randrange(R) for _ in range(n_inputs)]


def random_program(seed, n_instr=300, n_inputs=5, n_vars=24, holding=True):
    """A program of about n_instr instructions that uses every opcode, with BIT at indices 0 and 253, INV0 of a wire that is 0
    and of wires that are not, and ASSERT_ZERO statements.  holding=True: every assertion is over a wire that is zero for all
    inputs (x - x), so every instance succeeds; False: two assertions over arbitrary wires are added (most inputs violate both, and
    the earlier one must be the one reported)."""
    rng = random.Random(seed)
    consts = [0, 1, 2, R - 1, rng.randrange(R), rng.randrange(R)]
    instrs, n_stmt = [], 0
    wire = [1 + n_inputs]          # the next wire

    def emit(op, a=0, b=0):
        instrs.append((op, a, b, 0))
        if op != ASSERT_ZERO:
            wire[0] += 1
            return wire[0] - 1

    def any_wire():
        return rng.randrange(wire[0])

    zero = emit(SUB, 1, 1)                               # x - x
    emit(INV0, zero)                                     # INV0 of a wire that is 0
    emit(BIT, 1, 0)
    emit(BIT, 1, 253)
    emit(BIT, 2, 253)
    emit(CONST, 3)
    emit(BIT, wire[0] - 1, 253)                          # r - 1 has bit 253 set
    emit(ASSERT_ZERO, zero, n_stmt); n_stmt += 1
    free = []
    while len(instrs) < n_instr:
        op = rng.choice((CONST, ADD, ADD, SUB, SUB, MUL, MUL, MUL, INV0, BIT, BIT, ASSERT_ZERO))
        if op == CONST:
            emit(op, rng.randrange(len(consts)))
        elif op in (ADD, SUB, MUL):
            emit(op, any_wire(), any_wire())
        elif op == INV0:
            emit(op, any_wire())
        elif op == BIT:
            a = any_wire()
            for i in sorted(rng.sample(range(254), rng.choice((1, 3)))):   # runs over one wire, as num2bits makes them
                emit(op, a, i)
        else:
            a = any_wire()
            z = emit(SUB, a, a)
            emit(ASSERT_ZERO, z, n_stmt); n_stmt += 1
            if not holding and len(free) < 2 and len(instrs) > n_instr // 3:
                free.append(n_stmt)
                emit(ASSERT_ZERO, emit(MUL, any_wire(), 2), n_stmt); n_stmt += 1   # over wire x input 2: rarely zero
    sigmap = [0] + [rng.randrange(wire[0]) for _ in range(n_vars - 2)] + [wire[0] - 1]
    return encode(n_inputs, consts, instrs, sigmap, min(3, n_vars - 1), n_stmt)
