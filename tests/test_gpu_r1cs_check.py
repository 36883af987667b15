"""GPU: witnesses checked against their R1CS on the device before proving (zkr_r1cs_check / _check_device / _matches_key).

The expected failing sets are computed HERE with Python integers, constraint by constraint as oracle/groth16.check_r1cs does,
never taken from the library.  Base system: synth_circuit(2048, 7, 0x5A4B0001) -- 2048 signals, 2040 constraints, constraint
1000 the only wide one (63 A terms: the wavefront path), 56 constraints with an empty C (the first is 32), max(w) + r < 2^256."""
import pytest

import groth16 as g
from test_rollup import as_inputs, first_violated, ints, parse_r1cs, scenario

pytestmark = pytest.mark.gpu

R = g.R
SEED = 0x5A4B0001


def _r1cs(circ, rows=None, n_public=None):
    import zkr_hip
    rows = circ["rows"] if rows is None else rows
    return zkr_hip.binarify_r1cs(dict(nVars=circ["nVars"], nPublic=circ["nPublic"] if n_public is None else n_public,
                                      constraints=[[dict(lc) for lc in row] for row in rows]))


def _wb(w):
    return b"".join(int(x).to_bytes(32, "little") for x in w)


def _violated(rows, w):
    """The constraints `w` (any integers; reduced mod r as the prover reduces them) violates, in order."""
    ev = lambda lc: sum(cf * w[s] for s, cf in lc) % R
    return [i for i, (a, b, c) in enumerate(rows) if ev(a) * ev(b) % R != ev(c)]


def _report(rows, w):
    bad = _violated(rows, w)
    return {"violated": len(bad), "first": bad[0] if bad else None, "one_ok": w[0] % R == 1}


CLEAN = {"violated": 0, "first": None, "one_ok": True}


@pytest.fixture(scope="module")
def base():
    import zkr_hip
    circ = g.synth_circuit(2048, 7, SEED)
    rows, w = circ["rows"], circ["witness"]
    assert circ["nVars"] == 2048 and len(rows) == 2040 and g.check_r1cs(circ)
    assert [i for i, (a, b, c) in enumerate(rows) if max(len(a), len(b), len(c)) > 8] == [1000] and len(rows[1000][0]) == 63
    empty_c = [i for i, row in enumerate(rows) if not row[2]]
    assert len(empty_c) == 56 and empty_c[0] == 32 and max(w) + R < 1 << 256
    r1cs = _r1cs(circ)
    cs = zkr_hip.ConstraintSystem.load(r1cs)
    yield dict(circ=circ, rows=rows, w=w, r1cs=r1cs, cs=cs)
    cs.close()


def _rows_with(rows, i, side, k, delta=1):
    """A copy of the rows with `delta` added to the coefficient of term k of side `side` of constraint i."""
    out = [tuple(list(lc) for lc in row) for row in rows]
    s, cf = out[i][side][k]
    out[i][side][k] = (s, (cf + delta) % R)
    return out


def test_the_clean_witness_is_satisfied(base):                                               # (a)
    assert base["cs"].info() == {"nVars": 2048, "nPublic": 7, "nConstraints": 2040, "nnzA": sum(len(r[0]) for r in base["rows"]),
                                 "nnzB": sum(len(r[1]) for r in base["rows"]), "nnzC": sum(len(r[2]) for r in base["rows"])}
    assert base["cs"].check([_wb(base["w"])]) == (True, [CLEAN])


@pytest.mark.parametrize("s,want", [(1, None), (500, [492, 493, 506]), (1008, [1000, 1001, 1754]), (2047, [2039])])
def test_a_damaged_witness_word_is_located(base, s, want):                                    # (b)
    import zkr_hip
    w = list(base["w"])
    w[s] += 1
    bad = _violated(base["rows"], w)
    if want is None:
        assert len(bad) == 10 and bad[0] == 1
    else:
        assert bad == want
    ok, rep = base["cs"].check([_wb(w)])
    assert ok is False and rep == [{"violated": len(bad), "first": bad[0], "one_ok": True}]
    msg = zkr_hip.lib().zkr_last_error().decode()
    assert msg == "witness 0: %d constraints violated, first %d" % (len(bad), bad[0])


def test_signal_zero_must_be_one(base):                                                       # (b)
    import zkr_hip
    w = list(base["w"])
    w[0] = 2
    want = _report(base["rows"], w)
    assert want["one_ok"] is False
    ok, rep = base["cs"].check([_wb(w)])
    assert ok is False and rep == [want]
    assert "witness 0: signal 0 is not 1" in zkr_hip.lib().zkr_last_error().decode()
    # a consistent witness with w[0] = 2 satisfies every constraint of a system without constants and still proves nothing
    import zkr_hip as z
    tiny = z.ConstraintSystem.load(z.binarify_r1cs(dict(nVars=2, nPublic=0, constraints=[[[(1, 1)], [(1, 1)], [(1, 1)]]])))
    assert tiny.check([_wb([2, 1])]) == (False, [{"violated": 0, "first": None, "one_ok": False}])
    tiny.close()


def test_words_above_r_get_the_verdict_of_their_residue(base):                                # (b)
    w = [x + R for x in base["w"]]
    assert all(x < 1 << 256 for x in w)
    assert base["cs"].check([_wb(w)]) == (True, [CLEAN])
    w[500] += 1                                            # and a violated one stays violated under the same shift
    bad = _violated(base["rows"], w)
    assert bad == [492, 493, 506]
    assert base["cs"].check([_wb(w)]) == (False, [{"violated": 3, "first": 492, "one_ok": True}])


@pytest.mark.parametrize("i,side,k", [(1000, 0, -1), (0, 1, 0), (2039, 2, 0)])
def test_a_damaged_coefficient_fails_exactly_its_constraint(base, i, side, k):               # (c)
    import zkr_hip
    sig = base["rows"][i][side][k][0]
    assert base["w"][sig] % R != 0
    rows = _rows_with(base["rows"], i, side, k)
    assert _violated(rows, base["w"]) == [i]
    cs = zkr_hip.ConstraintSystem.load(_r1cs(base["circ"], rows))
    assert cs.check([_wb(base["w"])]) == (False, [{"violated": 1, "first": i, "one_ok": True}])
    cs.close()


def test_more_than_one_stride_of_a_wavefront_and_a_wide_c(base):                              # (d)
    import zkr_hip
    w = base["w"]
    rng = g.SplitMix64(0xD1D1)
    a = [(1 + 13 * j, rng.fr()) for j in range(150)]       # 150 distinct signals: three strides of 64 lanes, the last one partial
    c = [(3 + 29 * j, rng.fr()) for j in range(69)]
    last = 2046
    assert len({s for s, _ in a}) == 150 and len({s for s, _ in c} | {last}) == 70 and max(s for s, _ in a) < 2048 and w[last] % R != 0
    ev = lambda lc: sum(cf * w[s] for s, cf in lc) % R
    solved = (ev(a) * w[0] - ev(c)) * pow(w[last], -1, R) % R
    rows = list(base["rows"]) + [(a, [(0, 1)], c + [(last, solved)])]
    assert _violated(rows, w) == []
    cs = zkr_hip.ConstraintSystem.load(_r1cs(base["circ"], rows))
    assert cs.info()["nConstraints"] == 2041 and cs.check([_wb(w)]) == (True, [CLEAN])
    cs.close()
    rows[-1] = (a, [(0, 1)], c + [(last, (solved + 1) % R)])
    assert _violated(rows, w) == [2040]
    cs = zkr_hip.ConstraintSystem.load(_r1cs(base["circ"], rows))
    assert cs.check([_wb(w)]) == (False, [{"violated": 1, "first": 2040, "one_ok": True}])
    cs.close()


def test_a_batch_reports_per_witness_and_device_witnesses_agree_with_host_bytes(base):       # (e)
    import torch
    import zkr_hip
    ws = []
    for seed in (1, 2, 3):
        c = g.synth_circuit(2048, 7, SEED, witness_seed=seed)
        assert c["rows"] == base["rows"] and g.check_r1cs(c)
        ws.append(list(c["witness"]))
    ws[1][500] += 1
    want = [_report(base["rows"], w) for w in ws]
    assert want[0] == CLEAN and want[2] == CLEAN and want[1]["violated"] >= 1
    host = [_wb(w) for w in ws]
    assert base["cs"].check(host) == (False, want)
    assert zkr_hip.lib().zkr_last_error().decode() == "witness 1: %d constraints violated, first %d" % (want[1]["violated"], want[1]["first"])
    dev = [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in host]
    got = base["cs"].check_device([t.data_ptr() for t in dev], stream=torch.cuda.current_stream().cuda_stream)
    assert got == (False, want)
    assert base["cs"].check_device([dev[0].data_ptr(), dev[2].data_ptr()]) == (True, [CLEAN, CLEAN])


def test_the_smallest_system(base):                                                           # (f)
    import zkr_hip
    cs = zkr_hip.ConstraintSystem.load(zkr_hip.binarify_r1cs(dict(nVars=2, nPublic=1, constraints=[[[(1, 1)], [(1, 1)], [(1, 1)]]])))
    assert cs.info() == {"nVars": 2, "nPublic": 1, "nConstraints": 1, "nnzA": 1, "nnzB": 1, "nnzC": 1}
    assert cs.check([_wb([1, 1])]) == (True, [CLEAN])
    assert cs.check([_wb([1, 2])]) == (False, [{"violated": 1, "first": 0, "one_ok": True}])
    assert cs.check([_wb([1, 1]), _wb([1, 2]), _wb([1, 0])]) == (False, [CLEAN, {"violated": 1, "first": 0, "one_ok": True}, CLEAN])
    with pytest.raises(zkr_hip.ZkrError) as e:
        cs.check([_wb([1, 1, 1])])
    assert e.value.code == -3
    cs.close()


def test_the_tx_circuit_device_to_device():                                                   # (g)
    import torch
    import zkr_hip
    from zkr_hip import rollup as n
    c = n.RollupCircuit(2, 6)
    r1cs = c.r1cs()
    cs = zkr_hip.ConstraintSystem.load(r1cs)
    flats = [as_inputs(scenario(2, 6, seed, n_accounts=5)[0]) for seed in (41, 42, 44, 45)]
    dev = c.calculate_witness_batch_device(flats)
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = [dev[i].data_ptr() for i in range(4)]
    assert cs.check_device(ptrs, stream=stream) == (True, [CLEAN] * 4)
    nv, npub, cons = parse_r1cs(r1cs)
    s = npub + 1 + (nv - npub - 1) // 2                    # a private signal
    w = ints(bytes(dev[2].cpu().numpy().tobytes()))
    w[s] = (w[s] + 1) % R
    dev[2, 32 * s:32 * s + 32] = torch.frombuffer(bytearray(w[s].to_bytes(32, "little")), dtype=torch.uint8).cuda()
    first = first_violated(cons, w, R)
    assert first >= 0
    ok, rep = cs.check_device(ptrs, stream=stream)
    assert ok is False and [r["violated"] == 0 for r in rep] == [True, True, False, True] and all(r["one_ok"] for r in rep)
    assert rep[2]["first"] == first and rep[2]["violated"] == len(_violated(cons, w))
    cs.close()


def test_matches_key(base, small_case):                                                       # (h)
    import zkr_hip
    circ, rows = base["circ"], base["rows"]
    key, _ = zkr_hip.ProvingKey.setup_r1cs(base["r1cs"], toxic=[2, 3, 5, 7, 11])
    assert base["cs"].matches_key(key) is True
    ws = zkr_hip.ProvingKey.load_websnark(small_case["pkb"])            # a key the oracle built by another route
    cs_small = zkr_hip.ConstraintSystem.load(_r1cs(small_case["circ"]))
    assert cs_small.matches_key(ws) is True
    assert cs_small.matches_key(key) is False and "nVars" in zkr_hip.lib().zkr_last_error().decode()
    other_a = zkr_hip.ConstraintSystem.load(_r1cs(circ, _rows_with(rows, 1234, 0, 0)))
    assert other_a.matches_key(key) is False
    assert "side A" in zkr_hip.lib().zkr_last_error().decode() and "first 1234" in zkr_hip.lib().zkr_last_error().decode()
    other_b = zkr_hip.ConstraintSystem.load(_r1cs(circ, _rows_with(rows, 2039, 1, 0)))
    assert other_b.matches_key(key) is False and "side B" in zkr_hip.lib().zkr_last_error().decode()
    other_p = zkr_hip.ConstraintSystem.load(_r1cs(circ, n_public=8))
    assert other_p.matches_key(key) is False
    other_c = zkr_hip.ConstraintSystem.load(_r1cs(circ, _rows_with(rows, 2039, 2, 0)))
    assert other_c.matches_key(key) is True                # the documented limit: a key has no C side to compare
    for x in (other_a, other_b, other_p, other_c, cs_small):
        x.close()
