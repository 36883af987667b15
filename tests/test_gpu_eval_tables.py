"""GPU: the side tables of the evaluation form derived from a key's OWN points (include/zkr.h zkr_key_eval_tables,
csrc/zkr_eval_tables.hip), for the keys a deployment proves with: loaded from websnark bytes or a file, made from a transcript,
replicated, contributed to.

Every case has a scalar-knowing twin: zkr_setup_r1cs with the toxic scalars injected builds the same two tables from the scalars
(workload.hip key_build_eval_tables).  Affine canonical points are unique and the window levels are a function of level 0, so the
derived tables must be the twin's BYTES (eval_tables_equal), and `derived.eval_tables(r1cs)` must answer exactly as the twin's
builder did.  Proofs are compared with the closed form from the toxic scalars and with the C oracle on the websnark rendering of
the same setup, byte for byte.

Sizes: domain 2^7 (one wavefront per launch would hide nothing: 128 butterflies are two, and the tables have 128 to 505 points, more
than one workgroup of the per-slot addition) except the column that must not fit one combine task, which needs 300 rows: 2^9."""
import random

import pytest

import coracle
import groth16 as g
from bn254 import Q, R
import bn254 as b

pytestmark = pytest.mark.gpu

TOX = ("t", "alfa", "beta", "gamma", "delta")
MONT = 1 << 256
EVAL, COEF = "evaluation", "coefficients"


def _r1cs(circ):
    import zkr_hip
    return zkr_hip.binarify_r1cs(dict(nVars=circ["nVars"], nPublic=circ["nPublic"], constraints=[[list(lc) for lc in row] for row in circ["rows"]]))


def _case(circ, tox=None):
    """The twin (setup_r1cs with the toxic scalars), the websnark rendering of the same setup and a key loaded from it."""
    import zkr_hip
    tox = tox or g.toxic_from_seed(0x5A4B00FF)
    r1cs = _r1cs(circ)
    toxic = [tox[k] for k in TOX]
    twin, vk = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=toxic)
    pkb, _ = zkr_hip.setup_r1cs_websnark(r1cs, toxic=toxic)
    return dict(circ=circ, tox=tox, r1cs=r1cs, twin=twin, vk=vk, pkb=pkb, key=zkr_hip.ProvingKey.load_websnark(pkb), w=circ["witness"],
                wb=g.binarify_witness(circ["witness"]))


def _closed(c, r, s, tox=None):
    return g.proof_bytes(g.proof_from_toxic(c["circ"], tox or c["tox"], c["w"], r, s))


def _close(c):
    c["twin"].close()
    c["key"].close()


def _derive_as_the_twin(key, c):
    """derived.eval_tables answers as the twin's builder did; when both built, the tables are the twin's bytes."""
    built = key.eval_tables(c["r1cs"])
    twin_form = c["twin"].h_form()["form"]
    assert built == (twin_form == EVAL)
    assert key.h_form()["form"] == (EVAL if built else COEF)
    assert key.eval_tables_equal(c["twin"]) == built and c["twin"].eval_tables_equal(key) == built
    return built


@pytest.fixture(scope="module")
def small():
    c = _case(g.synth_circuit(128, 7, 0x5A4B0001))
    yield c
    _close(c)


def _last_error():
    import zkr_hip
    return zkr_hip.lib().zkr_last_error().decode()


# ---------------------------------------------------------------- 1. a key loaded from websnark bytes
def test_websnark_key_takes_the_evaluation_form_and_gives_it_back(small):
    c, key = small, small["key"]
    r, s = 0x1234567890ABCDEF, 0x0FEDCBA987654321
    assert key.h_form() == {"form": COEF, "retries": 0}
    p0 = key.prove(c["wb"], r, s)
    assert _derive_as_the_twin(key, c) is True
    assert key.prove(c["wb"], r, s) == p0 == _closed(c, r, s) == coracle.prove(c["pkb"], c["wb"], r, s)
    assert key.h_form() == {"form": EVAL, "retries": 0}        # a satisfying witness is proved once
    rnd = random.Random(71)
    bad = g.binarify_witness([1] + [rnd.randrange(R) for _ in range(len(c["w"]) - 1)])
    assert key.prove(bad, r, s) == coracle.prove(c["pkb"], bad, r, s)
    assert key.h_form() == {"form": EVAL, "retries": 1}        # proved again through the coefficient form
    key.drop_eval_tables()
    assert key.h_form()["form"] == COEF and not key.eval_tables_equal(c["twin"])
    assert key.prove(c["wb"], r, s) == p0
    key.drop_eval_tables()                                      # nothing to drop: fine
    assert _derive_as_the_twin(key, c) is True                  # again
    assert _derive_as_the_twin(key, c) is True                  # over tables that are there: dropped first, rebuilt
    assert key.prove(c["wb"], r, s) == p0


# ---------------------------------------------------------------- 2. a C column that does not fit one combine task
def _long_c_column():
    """Domain 2^9, one public signal.  Signal 0 sits on the C side of 300 rows with full-width coefficients: more than the 256 terms
    and far more than the 512 ladder steps of one combine task (zkr_ptau.hip COMBINE_TASK_TERMS / _STEPS), so its column is cut
    into partial sums that further launches add.  The public signal sits on the C side of 40 rows.  Each row's new signal absorbs
    what the extra terms add, as _public_in_c of tests/test_gpu_eval_h.py does."""
    rnd = random.Random(0x5A4B0900)
    p, m = 1, 512
    w = [1, rnd.randrange(1, R)]
    rows = []
    for row in range(m - p - 1):
        n = len(w)
        A = sorted({n - 1: 1, rnd.randrange(n): rnd.randrange(1, R)}.items())
        B = [(rnd.randrange(n), rnd.randrange(1, R))]
        val = sum(cf * w[s] for s, cf in A) * sum(cf * w[s] for s, cf in B) % R
        C = []
        if row < 300:
            cf = rnd.randrange(1 << 252, R)
            C.append((0, cf))
            val = (val - cf * w[0]) % R
        if row % 12 == 5 and row < 480:
            cf = rnd.randrange(1, R)
            C.append((1, cf))
            val = (val - cf * w[1]) % R
        rows.append((A, B, C + [(n, 1)]))
        w.append(val)
    circ = dict(nVars=len(w), nPublic=p, nConstraints=len(rows), domainSize=m, rows=rows, witness=w)
    assert g.check_r1cs(circ)
    assert sum(1 for _, _, C in rows if any(s == 0 for s, _ in C)) == 300 and sum(1 for _, _, C in rows if any(s == 1 for s, _ in C)) == 40
    return circ


def test_a_c_column_cut_into_partial_sums():
    c = _case(_long_c_column())
    try:
        assert c["twin"].h_form()["form"] == EVAL and c["key"].info()["domainSize"] == 512
        assert _derive_as_the_twin(c["key"], c) is True
        r, s = 77, 99
        assert c["key"].prove(c["wb"], r, s) == _closed(c, r, s) == coracle.prove(c["pkb"], c["wb"], r, s)
        assert c["key"].h_form()["retries"] == 0
    finally:
        _close(c)


# ---------------------------------------------------------------- 3. a transcript key, before and after a delta contribution
def test_transcript_key_and_the_key_contributed_to(small):
    import zkr_hip
    from test_gpu_ptau import ALFA, BETA, D, TAU, _transcript
    circ, r1cs, wb = small["circ"], small["r1cs"], small["wb"]
    pub = small["w"][1:8]
    k0, vk0 = zkr_hip.ProvingKey.setup_r1cs_ptau(r1cs, _transcript(7))
    t0, _ = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=[TAU, ALFA, BETA, 1, 1])
    t1, _ = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=[TAU, ALFA, BETA, 1, D])
    k1 = None
    try:
        assert k0.h_form()["form"] == COEF and t0.h_form()["form"] == EVAL and t1.h_form()["form"] == EVAL
        assert k0.eval_tables(r1cs) is True and k0.eval_tables_equal(t0) and not k0.eval_tables_equal(t1)
        k1, rec = k0.contribute(D)
        assert k0.h_form()["form"] == EVAL and k1.h_form() == {"form": COEF, "retries": 0}     # as before: a contributed key comes without
        assert k1.eval_tables(r1cs) is True and k1.eval_tables_equal(t1) and not k1.eval_tables_equal(t0)
        r, s = 3, 4
        proof = k1.prove(wb, r, s)
        assert proof == g.proof_bytes(g.proof_from_toxic(circ, dict(t=TAU, alfa=ALFA, beta=BETA, gamma=1, delta=D), circ["witness"], r, s))
        assert k1.h_form() == {"form": EVAL, "retries": 0}
        assert zkr_hip.verify(zkr_hip.vk_contribute(vk0, rec), proof, pub) is True and zkr_hip.verify(vk0, proof, pub) is False
    finally:
        for k in (k0, k1, t0, t1):
            if k is not None:
                k.close()


# ---------------------------------------------------------------- 4. layouts
def test_c_and_h_reduced_apart():
    """100 signals under a domain of 2^8 (tests/layout_cases.py): C' takes C's plan (window 7), E' takes H's (window 8)."""
    from layout_cases import few_signals_many_constraints
    lc = few_signals_many_constraints()
    c = _case(lc["circ"])
    try:
        win = c["key"].windows()
        assert win["C"][0] == 7 and win["H"][0] == 8
        built = _derive_as_the_twin(c["key"], c)
        assert built is True
        r, s = 5, 7
        assert c["key"].prove(c["wb"], r, s) == _closed(c, r, s) == coracle.prove(lc["pkb"], c["wb"], r, s)   # the oracle on the ORACLE's setup
    finally:
        _close(c)


def _public_signal_without_a_slot():
    """Domain 2^7, three public signals.  The A side reads the first eight signals only, so the supports of A and C overlap in a
    handful of signals and the two tables are NOT laid out over their union: C's accumulation reads C's own points, which are
    the private signals'.  Every third row carries a public signal on its C side: its C' point is finite and has no slot."""
    rnd = random.Random(0x5A4B0400)
    p, m = 3, 128
    w = [1] + [rnd.randrange(1, R) for _ in range(p)]
    rows = []
    for row in range(m - p - 1):
        n = len(w)
        A = [(rnd.randrange(min(n, 8)), rnd.randrange(1, R))]
        B = sorted({n - 1: 1, rnd.randrange(n): rnd.randrange(1, R)}.items())
        val = sum(cf * w[s] for s, cf in A) * sum(cf * w[s] for s, cf in B) % R
        C = []
        if row % 3 == 0:
            pub, cf = 1 + rnd.randrange(p), rnd.randrange(1, R)
            C.append((pub, cf))
            val = (val - cf * w[pub]) % R
        rows.append((A, B, C + [(n, 1)]))
        w.append(val)
    circ = dict(nVars=len(w), nPublic=p, nConstraints=len(rows), domainSize=m, rows=rows, witness=w)
    assert g.check_r1cs(circ)
    return circ


def test_a_public_signal_of_c_without_a_slot_leaves_the_coefficient_form():
    c = _case(_public_signal_without_a_slot())
    try:
        info = c["key"].info()
        assert info["ptsA"] != info["ptsC"]                      # not one support: C is sorted on its own
        assert c["twin"].h_form()["form"] == COEF                # the scalar-knowing builder gave up
        assert _derive_as_the_twin(c["key"], c) is False         # ... and so does the derivation, for the reason it names
        assert "not built" in _last_error() and "no slot" in _last_error()
        r, s = 11, 13
        assert c["key"].prove(c["wb"], r, s) == _closed(c, r, s) == coracle.prove(c["pkb"], c["wb"], r, s)
        assert c["key"].h_form() == {"form": COEF, "retries": 0}
    finally:
        _close(c)


# ---------------------------------------------------------------- 5. a stale C side
def test_a_stale_c_side_costs_a_retry_per_proof_and_no_wrong_proof(small):
    """The same geometry with one C coefficient changed: the tables build (nothing binds the system to the key), no witness of
    the REAL circuit satisfies the changed row, and every proof is proved again through the coefficient form."""
    import zkr_hip
    c = small
    rows = [tuple(list(lc) for lc in row) for row in c["circ"]["rows"]]
    at = next(i for i, (_, _, C) in enumerate(rows) if C and c["w"][C[0][0]])   # a row whose C side is not zero for this witness
    s0, cf0 = rows[at][2][0]
    rows[at][2][0] = (s0, (cf0 + 1) % R)
    stale = _r1cs(dict(c["circ"], rows=rows))
    assert stale != c["r1cs"] and len(stale) == len(c["r1cs"])
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    try:
        assert key.eval_tables(stale) is True and key.h_form() == {"form": EVAL, "retries": 0}
        assert not key.eval_tables_equal(c["twin"])
        wits = [c["wb"]] + [zkr_hip.synth_witness(7, 7, 0x5A4B0001, 900 + i) for i in (1, 2)]
        for i, wb in enumerate(wits):
            assert key.prove(wb, 21 + i, 31 + i) == coracle.prove(c["pkb"], wb, 21 + i, 31 + i)
            assert key.h_form()["retries"] == i + 1
    finally:
        key.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(small):
    import torch
    import zkr_hip
    c = small
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    shard = key.shard(0, 2)
    try:
        other = _r1cs(g.synth_circuit(64, 7, 0x5A4B0001))
        for k, r1cs, what in ((key, other, "nVars"), (shard, c["r1cs"], "shard")):
            with pytest.raises(zkr_hip.ZkrError) as e:
                k.eval_tables(r1cs)
            assert e.value.code == -5 and what in str(e.value)
        assert key.h_form()["form"] == COEF
        # between submit and collect: refused, and the ticket collects as if nothing had been asked
        d_w = torch.frombuffer(bytearray(c["wb"]), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        r, s = 41, 43
        ticket = key.prove_submit(d_w.data_ptr(), r, s)
        with pytest.raises(zkr_hip.ZkrError) as e:
            key.eval_tables(c["r1cs"])
        assert e.value.code == -5 and "in flight" in str(e.value)
        assert key.prove_collect(ticket) == _closed(c, r, s)
        assert key.h_form()["form"] == COEF
        assert key.eval_tables(c["r1cs"]) is True                # collected: now it builds
        ticket = key.prove_submit(d_w.data_ptr(), r, s)
        with pytest.raises(zkr_hip.ZkrError) as e:
            key.drop_eval_tables()
        assert e.value.code == -5 and "in flight" in str(e.value)
        assert key.prove_collect(ticket) == _closed(c, r, s) and key.h_form() == {"form": EVAL, "retries": 0}
    finally:
        shard.close()
        key.close()


# ---------------------------------------------------------------- 7. neighbours: files and replicas carry no tables
def test_files_and_replicas_carry_no_tables_and_derive_their_own(small, tmp_path):
    import zkr_hip
    c = small
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    loaded = replica = None
    try:
        key.save(str(tmp_path / "before.zkr"))
        assert key.eval_tables(c["r1cs"]) is True
        key.save(str(tmp_path / "after.zkr"))
        assert open(tmp_path / "before.zkr", "rb").read() == open(tmp_path / "after.zkr", "rb").read()
        loaded = zkr_hip.ProvingKey.load_file(str(tmp_path / "after.zkr"))
        replica = key.replicate(0)
        r, s = 51, 53
        for k in (loaded, replica):
            assert k.h_form() == {"form": COEF, "retries": 0} and not k.eval_tables_equal(key)
            assert _derive_as_the_twin(k, c) is True and k.eval_tables_equal(key)
            assert k.prove(c["wb"], r, s) == _closed(c, r, s)
    finally:
        for k in (key, loaded, replica):
            if k is not None:
                k.close()


# ---------------------------------------------------------------- 8. the per-slot addition against the oracle
def _le(v):
    return int(v).to_bytes(32, "little")


def _mont(P, g2):
    if P is None:
        return bytes(128 if g2 else 64)
    cs = (P[0][0], P[0][1], P[1][0], P[1][1]) if g2 else P
    return b"".join(_le(x * MONT % Q) for x in cs)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_points_add_each_matches_the_oracle(g2):
    """70 entries, more than one wavefront: P + Q, P + P, P + (-P), O + Q, P + O, O + O in turn, with infinity given as all zeros
    and as the wire form (x = 0, y = one); the sum at infinity comes back as all zeros."""
    import zkr_hip
    fb = g._fb()[1 if g2 else 0]
    add, neg = (b.g2_add, b.g2_neg) if g2 else (b.g1_add, b.g1_neg)
    rng = g.SplitMix64(0x5A4B0800 + g2)
    pts = [fb.mul(rng.fr()) for _ in range(24)]
    wire_inf = (bytes(64) + _le(MONT % Q) + bytes(32)) if g2 else (bytes(32) + _le(MONT % Q))
    A, B, want = [], [], []
    for i in range(70):
        P, S = pts[i % 24], pts[(7 * i + 3) % 24]
        a, s = [(P, S), (P, P), (P, neg(P)), (None, S), (P, None), (None, None)][i % 6]
        if i % 6 == 0:
            assert P != S
        A.append(wire_inf if a is None and i % 12 >= 6 else _mont(a, g2))
        B.append(wire_inf if s is None and i % 12 >= 6 else _mont(s, g2))
        want.append(_mont(add(a, s), g2))
    out = zkr_hip.points_add_each(b"".join(A), b"".join(B), g2=g2)
    pb = 128 if g2 else 64
    bad = [i for i in range(70) if out[pb * i:pb * i + pb] != want[i]]
    assert bad == []
    assert want[2] == bytes(pb) and want[5] == bytes(pb) and want[1] != bytes(pb)
