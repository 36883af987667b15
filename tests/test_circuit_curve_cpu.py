"""CPU: the builder's hint values, its BabyJub gadgets and the Ecdh circuit (zkr_hip.circuit; prover/circuits/ecdh.circom, whose
test prover/__tests__/ecdh.test.ts asks sharedKey == ecdh) through the engine's host twin (zkr_hip.wprog_run_host) and the Python
interpreter of tests/wprog_model.py, against oracle/rollup.py's curve and tests/crypto_model.py."""
import functools
import random
import struct

import pytest

import crypto_model as m
import rollup as o
import wallet_cases as wc
import wprog_model as wm
import zkr_hip
from zkr_hip import circuit as C

R = o.R
OFF_CURVE = (1, 1)


def _ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _r1cs_rows(blob):
    n_vars, n_public, n_c = struct.unpack_from("<III", blob, 0)
    off, rows = 12, []
    for _ in range(n_c):
        row = []
        for _side in range(3):
            k, = struct.unpack_from("<I", blob, off)
            off += 4
            row.append([(struct.unpack_from("<I", blob, off + 36 * t)[0], int.from_bytes(blob[off + 36 * t + 4:off + 36 * t + 36], "little")) for t in range(k)])
            off += 36 * k
        rows.append(row)
    assert off == len(blob)
    return n_vars, n_public, rows


def _first_violated(rows, witness):
    dot = lambda terms: sum(c * witness[s] for s, c in terms) % R
    for k, (a, b, c) in enumerate(rows):
        if dot(a) * dot(b) % R != dot(c):
            return k
    return None


def _run(blob, row):
    """the host twin's run, which must also be the Python interpreter's"""
    run = zkr_hip.wprog_run_host(blob, row)
    w = _ints(run.witness)
    code, stmt, _, want = wm.run(blob, row)
    assert (run.code, w) == (code, want) and (code == 0 or run.statement == stmt)
    return run, w


@functools.lru_cache(maxsize=None)
def ecdh_circuit():
    c = C.Ecdh()
    return c, c.program(), _r1cs_rows(c.r1cs())[2]


def _neg(p):
    return ((R - p[0]) % R, p[1])


def test_hint_values_emit_no_constraint_and_witness_names_them():
    c = C.Circuit()
    out = c.output("q")
    x, y = c.public_input("x"), c.private_input("y")
    h = (c.hint(x) * 3 + c.hint(y - 1)) * c.hint(x + y).inv() - 2      # (3x + y - 1) / (x + y) - 2
    assert isinstance(h, C.Hint) and c.constraints == []
    q = c.witness(h, "quot")
    assert c.constraints == [] and c.n_vars == 5
    c.constrain(x + y, q + 2, x * 3 + y - 1)
    c.assign(out, q)
    assert c.counts()["INV0"] == 1
    rows = _r1cs_rows(c.r1cs())[2]
    run, w = _run(c.program(), [5, 9])
    assert run.code == 0 and w[1] == w[4] == ((3 * 5 + 8) * pow(14, R - 2, R) - 2) % R and _first_violated(rows, w) is None
    with pytest.raises(ValueError):
        c.witness(x)
    with pytest.raises(ValueError):
        C.Circuit().witness(h)


def test_babyjub_add_equals_the_oracle():
    c = C.Circuit()
    ox, oy = c.output("x"), c.output("y")
    p = (c.public_input("px"), c.public_input("py"))
    q = (c.public_input("qx"), c.public_input("qy"))
    x3, y3 = C.gadgets.babyjub_add(c, p, q)
    c.assign(ox, x3)
    c.assign(oy, y3)
    assert len(c.constraints) == 6 + 2 and c.counts()["INV0"] == 1
    blob, rows = c.program(), _r1cs_rows(c.r1cs())[2]
    rng = random.Random(0x5A4B0500)
    pts = [o.bj_mul(o.BASE8, rng.randrange(1, o.SUBORDER)) for _ in range(4)]
    ident = (0, 1)
    cases = [(pts[0], pts[1]), (pts[2], pts[3]), (pts[0], ident), (ident, pts[1]), (ident, ident), (pts[2], pts[2]), (pts[3], _neg(pts[3])),
             ((0, R - 1), pts[0])]
    for a, b in cases:
        assert o.bj_on_curve(a) and o.bj_on_curve(b)
        run, w = _run(blob, list(a) + list(b))
        assert run.code == 0 and (w[1], w[2]) == tuple(o.bj_add(a, b)), (a, b)
        assert _first_violated(rows, w) is None
    assert tuple(o.bj_add(pts[3], _neg(pts[3]))) == ident


def test_babyjub_dbl_and_check():
    c = C.Circuit()
    ox = c.output("x")
    p = (c.public_input("px"), c.public_input("py"))
    C.gadgets.babyjub_check(c, p, "p is on the curve")
    c.assign(ox, C.gadgets.babyjub_dbl(c, p)[0])
    blob, rows = c.program(), _r1cs_rows(c.r1cs())[2]
    pt = o.bj_mul(o.BASE8, 77)
    run, w = _run(blob, list(pt))
    assert run.code == 0 and w[1] == o.bj_add(pt, pt)[0] and _first_violated(rows, w) is None
    run, w = _run(blob, list(OFF_CURVE))
    assert (run.code, c.statements[run.statement]) == (2, "p is on the curve") and w == [0] * c.n_vars


def test_ecdh_circuit_shape():
    c, _, rows = ecdh_circuit()
    assert c.input_names == ["publicKey[0]", "publicKey[1]", "privateKey"] and c.n_public == 3 and len(c.privates) == 1
    assert c.statements == ["private key fits 253 bits", "public key is on the curve"]
    assert c.counts()["INV0"] <= 2
    per_bit = (len(rows) - 254 - 3 - 1) / 253.0   # without Num2Bits, the curve check and the output's row
    assert 13 <= per_bit <= 14, per_bit


def test_ecdh_circuit_gives_the_models_shared_key_and_satisfies_its_r1cs():
    c, blob, rows = ecdh_circuit()
    pubs = wc.oracle_pubs()
    base = pubs[3]
    for f in (0, 1, 2, 1 << 252, (1 << 253) - 1):
        run, w = _run(blob, [base[0], base[1], f])
        assert run.code == 0 and w[1] == o.bj_mul(base, f)[0], f
        assert w[0] == 1 and w[2:5] == [base[0], base[1], f] and _first_violated(rows, w) is None, f
    for t, (f, want) in enumerate(zip(wc.oracle_formatted(), m.list_shared_keys())):
        pub = pubs[(t + 1) % len(pubs)]
        run = zkr_hip.wprog_run_host(blob, [pub[0], pub[1], f])
        w = _ints(run.witness)
        assert run.code == 0 and w[1] == want, t
        if t % 16 == 0:
            assert _first_violated(rows, w) is None
    for pub in ((0, 1), (0, R - 1)):   # the identity and the point of order two
        run, w = _run(blob, [pub[0], pub[1], wc.oracle_formatted()[4]])
        assert run.code == 0 and w[1] == 0 and _first_violated(rows, w) is None
    bad = list(w)
    bad[1] = 1
    assert _first_violated(rows, bad) == len(rows) - 1   # sharedKey's own constraint is the last one


def test_ecdh_circuit_reports_a_long_key_and_an_off_curve_point():
    c, blob, _ = ecdh_circuit()
    base = wc.oracle_pubs()[3]
    run, w = _run(blob, [base[0], base[1], 1 << 253])
    assert (run.code, c.statements[run.statement]) == (2, "private key fits 253 bits") and w == [0] * c.n_vars
    run, w = _run(blob, [OFF_CURVE[0], OFF_CURVE[1], 5])
    assert (run.code, c.statements[run.statement]) == (2, "public key is on the curve") and w == [0] * c.n_vars
    run, w = _run(blob, [OFF_CURVE[0], OFF_CURVE[1], 1 << 253])   # both: the earlier statement
    assert (run.code, c.statements[run.statement]) == (2, "private key fits 253 bits")
