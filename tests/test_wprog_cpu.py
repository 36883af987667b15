"""CPU: witness programs (include/zkr.h wprog_bin; csrc/wprog.hpp) -- the validator's refusals one by one, the interpreter's host
twin against an independent Python interpreter (tests/wprog_model.py) wire for wire, and the circuit builder
(zkr_hip.circuit): what it emits as r1cs_bin is satisfied, row by row in Python integers, by what its program computes, and the
reference's wrapper circuits give the oracle's and the product's own hashes and roots."""
import random
import struct

import pytest

import wprog_model as m

R = m.R
ERR_ARG = -5


def _ints(b):
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


# ------------------------------------------------------------------------------------------------ validator
def _small():
    """inputs x, y; wires 3 CONST, 4 x + y, 5 (x + y) c, 6 bit 3 of x, 7 x - x; one assertion; four signals"""
    instrs = [(m.CONST, 1, 0, 0), (m.ADD, 1, 2, 0), (m.MUL, 4, 3, 0), (m.BIT, 1, 3, 0), (m.SUB, 1, 1, 0), (m.ASSERT_ZERO, 7, 0, 0)]
    return dict(n_inputs=2, consts=[5, 7], instrs=instrs, sigmap=[0, 5, 1, 6], n_public=1, n_statements=1)


def _refused(blob, *words):
    import zkr_hip
    with pytest.raises(zkr_hip.ZkrError) as e:
        zkr_hip.wprog_shape(blob)
    assert e.value.code == ERR_ARG
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    with pytest.raises(zkr_hip.ZkrError) as e2:   # the same answer from the load call, before it looks for a device
        zkr_hip.WitnessProgram(blob)
    assert e2.value.code == ERR_ARG and str(e2.value) == str(e.value)


def _with_instr(k, ins):
    p = _small()
    p["instrs"][k] = ins
    return m.encode(**p)


def test_the_undamaged_program_is_accepted_and_runs():
    import zkr_hip
    blob = m.encode(**_small())
    assert zkr_hip.wprog_shape(blob) == {"nInputs": 2, "nWires": 8, "nInstructions": 6, "nVars": 4, "nPublic": 1, "nStatements": 1}
    run = zkr_hip.wprog_run_host(blob, [9, 4], want_wires=True)
    assert (run.code, run.statement) == (0, 0)
    assert _ints(run.wires) == [1, 9, 4, 7, 13, 91, 1, 0] and _ints(run.witness) == [1, 91, 9, 1]


def test_validator_refuses_an_operand_equal_to_its_own_wire():
    _refused(_with_instr(1, (m.ADD, 4, 2, 0)), "instruction 1", "operand a = 4", "wire 4")
    _refused(_with_instr(1, (m.ADD, 1, 4, 0)), "instruction 1", "operand b = 4", "wire 4")
    _refused(_with_instr(5, (m.ASSERT_ZERO, 8, 0, 0)), "instruction 5", "operand a = 8")


def test_validator_refuses_bit_index_254():
    _refused(_with_instr(3, (m.BIT, 1, 254, 0)), "instruction 3", "bit index 254")
    import zkr_hip
    zkr_hip.wprog_shape(_with_instr(3, (m.BIT, 1, 253, 0)))


def test_validator_refuses_a_constant_equal_to_r():
    p = _small()
    p["consts"][1] = R
    _refused(m.encode(**p), "constant 1", "not below r")
    p["consts"][1] = R - 1
    import zkr_hip
    zkr_hip.wprog_shape(m.encode(**p))


def test_validator_refuses_a_constant_index_out_of_range():
    _refused(_with_instr(0, (m.CONST, 2, 0, 0)), "instruction 0", "constant index 2", "n_consts = 2")


def test_validator_refuses_a_map_entry_one_past_the_last_wire():
    p = _small()
    p["sigmap"][3] = 8
    _refused(m.encode(**p), "signal map entry 3 = 8", "wire count 8")


def test_validator_refuses_map_entry_0_that_is_not_wire_0():
    p = _small()
    p["sigmap"][0] = 1
    _refused(m.encode(**p), "signal map entry 0", "not wire 0")


def test_validator_refuses_a_length_short_or_long_by_one_byte():
    blob = m.encode(**_small())
    _refused(blob[:-1], "length is %d bytes" % (len(blob) - 1), "need %d" % len(blob))
    _refused(blob + b"\0", "length is %d bytes" % (len(blob) + 1), "need %d" % len(blob))


def test_validator_refuses_an_unknown_opcode():
    _refused(_with_instr(2, (8, 4, 3, 0)), "instruction 2", "opcode 8")
    _refused(_with_instr(2, (0, 4, 3, 0)), "instruction 2", "opcode 0")


def test_validator_refuses_an_unknown_version_and_magic():
    _refused(m.encode(version=2, **_small()), "version is 2")
    _refused(m.encode(magic=m.MAGIC + 1, **_small()), "magic")


def test_validator_refuses_n_public_not_below_n_vars_a_statement_out_of_range_and_counts_past_the_format():
    p = _small()
    p["n_public"] = 4
    _refused(m.encode(**p), "n_public = 4", "n_vars = 4")
    _refused(_with_instr(5, (m.ASSERT_ZERO, 7, 1, 0)), "instruction 5", "statement 1", "n_statements = 1")
    _refused(_with_instr(1, (m.ADD, 1, 2, 9)), "instruction 1", "operand c = 9")
    blob = bytearray(m.encode(**_small()))
    struct.pack_into("<I", blob, 8, (1 << 28) + 1)      # n_inputs: no byte of the file stands for an input, so only a limit stops it
    _refused(bytes(blob), "n_inputs", "limit")
    struct.pack_into("<I", blob, 8, (1 << 28) - 2)      # within the limit alone, past it with the instructions
    _refused(bytes(blob), "n_inputs", "n_instr", "limit")


# ------------------------------------------------------------------------------------------------ engine against the model
SEEDS = (1, 2, 3)


def _compare(blob, row):
    import zkr_hip
    code, stmt, wires, witness = m.run(blob, row)
    got = zkr_hip.wprog_run_host(blob, row, want_wires=True)
    assert (got.code, got.statement) == (code, stmt)
    assert _ints(got.wires) == wires
    assert _ints(got.witness) == witness
    return code, stmt


@pytest.mark.parametrize("seed", SEEDS)
def test_host_twin_equals_the_model_on_every_wire(seed):
    blob = m.random_program(seed)
    ops = {ins[0] for ins in m.decode(blob)["instrs"]}
    assert ops == {m.CONST, m.ADD, m.SUB, m.MUL, m.INV0, m.BIT, m.ASSERT_ZERO} and 280 <= len(m.decode(blob)["instrs"]) <= 320
    bits = {ins[2] for ins in m.decode(blob)["instrs"] if ins[0] == m.BIT}
    assert {0, 253} <= bits
    rng = random.Random(100 + seed)
    rows = [[v] * 5 for v in m.EDGE_VALUES] + [m.random_inputs(rng, 5) for _ in range(12)]
    for row in rows:
        assert _compare(blob, row) == (0, 0)


def test_an_input_equal_to_r_gives_code_1_with_the_inputs_index():
    blob = m.random_program(1)
    assert _compare(blob, [3, 4, R, 5, R]) == (1, 2)
    assert _compare(blob, [3, 4, 5, 6, (1 << 256) - 1]) == (1, 4)


def test_of_two_violated_assertions_the_earlier_one_is_reported():
    blob = m.random_program(7, holding=False)
    p = m.decode(blob)
    free = [ins[2] for k, ins in enumerate(p["instrs"]) if ins[0] == m.ASSERT_ZERO and p["instrs"][k - 1][0] == m.MUL]
    assert len(free) == 2 and free[0] < free[1]
    rng = random.Random(8)
    seen = set()
    for _ in range(12):
        row = [rng.randrange(2, R) for _ in range(5)]
        code, stmt, wires, _ = m.run(blob, row)
        both = all(wires[ins[1]] for ins in p["instrs"] if ins[0] == m.ASSERT_ZERO and ins[2] in free)
        assert _compare(blob, row) == (code, stmt)
        if both:
            assert (code, stmt) == (2, free[0])
            seen.add(stmt)
    assert seen == {free[0]}


# ------------------------------------------------------------------------------------------------ builder
def _r1cs_rows(blob):
    n_vars, n_public, n_c = struct.unpack_from("<III", blob, 0)
    off, rows = 12, []
    for _ in range(n_c):
        row = []
        for _side in range(3):
            k, = struct.unpack_from("<I", blob, off)
            off += 4
            terms = []
            for _t in range(k):
                s, = struct.unpack_from("<I", blob, off)
                terms.append((s, int.from_bytes(blob[off + 4:off + 36], "little")))
                off += 36
            row.append(terms)
        rows.append(row)
    assert off == len(blob)
    return n_vars, n_public, rows


def _first_violated(circuit, witness):
    n_vars, _, rows = _r1cs_rows(circuit.r1cs())
    assert n_vars == len(witness) == circuit.n_vars
    dot = lambda terms: sum(c * witness[s] for s, c in terms) % R
    for k, (a, b, c) in enumerate(rows):
        if dot(a) * dot(b) % R != dot(c):
            return k
    return None


def _run(circuit, row):
    import zkr_hip
    run = zkr_hip.wprog_run_host(circuit.program(), row)
    return run, _ints(run.witness)


def _tree(depth, leaves):
    import rollup as o
    t = o.Tree(depth)
    for i, v in leaves.items():
        t.update(i, v)
    return t


@pytest.mark.parametrize("length", (1, 2))
def test_hasher_witness_satisfies_its_r1cs_and_gives_the_oracles_hash(length):
    import rollup as o
    import zkr_hip.rollup as product
    from zkr_hip import circuit as C
    c = C.Hasher(length)
    assert c.n_public == length + 2 and c.input_names == ["in[%d]" % i for i in range(length)] + ["key"]
    ins = [R - 3, 12345678901234567890][:length]
    run, w = _run(c, ins + [0])
    assert run.code == 0 and w[0] == 1 and w[2:2 + length + 1] == ins + [0]        # one, output, then the public inputs in order
    assert _first_violated(c, w) is None
    assert w[1] == o.multi_hash(ins) == product.multi_hash(ins)
    run, w = _run(c, ins + [77])                                                   # the key input of hasher.circom
    assert _first_violated(c, w) is None and w[1] == o.multi_hash(ins, 77)
    bad = list(w)
    bad[1] = (bad[1] + 1) % R
    assert _first_violated(c, bad) == len(c.constraints) - 1                        # the output's own constraint is the last one


def test_hash_left_right_circuit():
    import rollup as o
    import zkr_hip.rollup as product
    from zkr_hip import circuit as C
    c = C.HashLeftRight()
    run, w = _run(c, [5, R - 1])
    assert run.code == 0 and _first_violated(c, w) is None
    assert w[1] == o.hash_left_right(5, R - 1) == product.hash_left_right(5, R - 1)
    assert len(c.constraints) == 2 * 3 * 220 + 1


@pytest.mark.parametrize("depth", (1, 2, 4))
def test_merkle_circuits_give_the_trees_root_and_refuse_a_wrong_leaf(depth):
    from zkr_hip import circuit as C
    idx = (1 << depth) - 2 if depth > 1 else 1
    t = _tree(depth, {idx: 4242, 0: 17})
    bits = [(idx >> l) & 1 for l in range(depth)]
    c = C.MerkleTreeRootConstructor(depth)
    assert c.n_public == 2 and len(c.privates) == 2 * depth
    run, w = _run(c, [4242] + t.path(idx) + bits)
    assert run.code == 0 and _first_violated(c, w) is None and w[1] == t.root
    run, w = _run(c, [4242] + t.path(idx) + [2] + bits[1:])                          # a path index that is no bit
    assert (run.code, c.statements[run.statement]) == (2, "path index 0 is 0 or 1") and w == [0] * c.n_vars
    e = C.MerkleTreeLeafExists(depth)
    assert e.n_public == 2 and e.input_names[:2] == ["leaf", "root"]
    run, w = _run(e, [4242, t.root] + t.path(idx) + bits)
    assert run.code == 0 and _first_violated(e, w) is None and w[1:3] == [4242, t.root]
    run, w = _run(e, [4243, t.root] + t.path(idx) + bits)
    assert (run.code, e.statements[run.statement]) == (2, "the leaf is in the tree with this root") and w == [0] * e.n_vars


def test_num2bits_is_zero_and_select():
    from zkr_hip import circuit as C
    c = C.Circuit()
    out = c.output("picked")
    x, a, b = c.public_input("x"), c.private_input("a"), c.private_input("b")
    bits = C.gadgets.num2bits(c, x, 253, "x fits 253 bits")
    z = C.gadgets.is_zero(c, a)
    c.assign(out, C.gadgets.select(c, z, b, a + bits[0] * 2))       # b when a is 0, a + 2 bit0(x) otherwise
    assert c.n_public == 2 and c.n_vars == 1 + 1 + 1 + 2 + 253 + 3
    sigs = c.signals()
    assert [s.kind for s in sigs[:5]] == ["one", "output", "public", "private", "private"] and {s.kind for s in sigs[5:]} == {"internal"}
    n_vars, n_public, rows = _r1cs_rows(c.r1cs())
    assert (n_vars, n_public) == (c.n_vars, c.n_public)
    for x_val, a_val, want in ((2 ** 253 - 1, 0, 9), (2 ** 253 - 2, 5, 5), (1, R - 1, 1)):
        run, w = _run(c, [x_val, a_val, 9])
        assert run.code == 0 and _first_violated(c, w) is None and w[1] == want
        assert w[5:5 + 253] == [(x_val >> i) & 1 for i in range(253)]
    run, w = _run(c, [2 ** 253, 0, 9])
    assert (run.code, c.statements[run.statement]) == (2, "x fits 253 bits")
    # booleanity and recomposition are IN the constraints: a witness with a bit set to 2 (recomposition kept) and one with a bit
    # flipped both fail, at the bit's own row and at the recomposition row
    run, w = _run(c, [6, 1, 9])
    two = list(w)
    two[5 + 1], two[5 + 2] = 3, 0                       # 6 = 0 + 3 * 2 + 0 * 4
    assert _first_violated(c, two) == 1
    flipped = list(w)
    flipped[5] = 1
    assert _first_violated(c, flipped) == 253


def test_round_constants_are_the_oracles():
    import rollup as o
    import zkr_hip
    assert zkr_hip.mimcsponge_round_constants() == o.mimc_constants()
