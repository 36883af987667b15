"""GPU: witness programs on the device (zkr_wprog_*, csrc/zkr_wprog.hip).  The device run equals the interpreter's host twin byte for
byte (which tests/test_wprog_cpu.py holds to the Python model wire for wire) across partial wavefronts and piece edges; a failing
instance is reported and zeroed and touches no other; and circuits stated with zkr_hip.circuit go witness -> check -> prove ->
verify without leaving device memory."""
import random

import pytest

import wprog_model as m

pytestmark = pytest.mark.gpu

R = m.R
SEEDS = (1, 2)


def _ints(b):
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


@pytest.fixture(scope="module")
def cases():
    """per seed: the program, 257 input rows, and the host twin's witness of each -- computed once"""
    import zkr_hip
    out = {}
    for seed in SEEDS:
        blob = m.random_program(seed)
        rng = random.Random(900 + seed)
        rows = [[v] * 5 for v in m.EDGE_VALUES] + [m.random_inputs(rng, 5) for _ in range(252)]
        runs = [zkr_hip.wprog_run_host(blob, row) for row in rows]
        assert all(r.code == 0 for r in runs)
        out[seed] = dict(blob=blob, rows=rows, want=[r.witness for r in runs])
    return out


@pytest.fixture(scope="module")
def progs(cases):
    import zkr_hip
    ps = {seed: zkr_hip.WitnessProgram(c["blob"], piece=64) for seed, c in cases.items()}
    yield ps
    for p in ps.values():
        p.close()


def _rows_bytes(t):
    return [bytes(r) for r in t.cpu().numpy()]


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("seed", SEEDS)
def test_device_equals_host_twin_byte_for_byte(cases, progs, seed, n):
    c, p = cases[seed], progs[seed]
    assert p.info()["piece"] == 64
    out = p.witness_batch_device(c["rows"][:n])
    assert tuple(out.shape) == (n, p.info()["nVars"] * 32)
    assert _rows_bytes(out) == c["want"][:n]
    assert p.reports == [(0, 0)] * n


def test_default_piece_gives_the_same_bytes_and_no_instance_is_nothing(cases):
    import torch
    import zkr_hip
    c = cases[1]
    p = zkr_hip.WitnessProgram(c["blob"])
    try:
        info = p.info()
        assert info["piece"] == 16384 and info["workspaceBytes"] == info["nWires"] * 16384 * 32 + 16384 * 8
        assert _rows_bytes(p.witness_batch_device(c["rows"])) == c["want"]
        none = p.witness_batch_device(torch.empty((0, 5 * 32), dtype=torch.uint8, device="cuda:0"))
        assert tuple(none.shape) == (0, info["nVars"] * 32) and p.witness_batch_device([]).shape[0] == 0
    finally:
        p.close()


@pytest.mark.parametrize("at", (0, 64, 256))
def test_a_failing_instance_stays_contained(at):
    """The program with two free assertions; every row but one is made to satisfy them (input 2 = 0 zeroes both asserted
    products), the row at `at` violates them.  Instances 0..63, 64..127, ... are separate pieces."""
    import zkr_hip
    blob = m.random_program(7, holding=False)
    rng = random.Random(70)
    good = [[rng.randrange(R), 0, rng.randrange(R), rng.randrange(R), rng.randrange(R)] for _ in range(257)]
    assert all(m.run(blob, row)[0] == 0 for row in good[:3] + [good[at]])
    bad_row = None
    while bad_row is None:
        row = [rng.randrange(2, R) for _ in range(5)]
        code, stmt, _, _ = m.run(blob, row)
        bad_row = row if code == 2 else None
    p = zkr_hip.WitnessProgram(blob, piece=64, statements=["statement %d of the test" % k for k in range(zkr_hip.wprog_shape(blob)["nStatements"])])
    try:
        clean = _rows_bytes(p.witness_batch_device(good))
        assert clean[at] == zkr_hip.wprog_run_host(blob, good[at]).witness
        rows = list(good)
        rows[at] = bad_row
        with pytest.raises(zkr_hip.ZkrError) as e:
            p.witness_batch_device(rows)
        assert e.value.code == -7 and str(e.value).endswith("instance %d violates: statement %d of the test" % (at, stmt))
        assert b"instance %d violates statement %d" % (at, stmt) in zkr_hip.lib().zkr_last_error()
        assert e.value.reports == [(2, stmt) if j == at else (0, 0) for j in range(257)]
        got = _rows_bytes(p.last)
        assert got[at] == bytes(len(got[at]))
        assert got[:at] + got[at + 1:] == clean[:at] + clean[at + 1:]
    finally:
        p.close()


def test_host_inputs_are_range_checked_before_anything_is_launched(cases, progs):
    import torch
    import zkr_hip
    c, p = cases[1], progs[1]
    rows = [list(r) for r in c["rows"][:70]]
    rows[66][3] = R
    rows[68][0] = R + 5
    before = p.witness_batch_device(c["rows"][:70]).clone()
    times = p.stage_times()
    assert times["run_ms"] > 0 and times["layout_ms"] > 0
    with pytest.raises(zkr_hip.ZkrError) as e:
        p.witness_batch_device(rows)
    assert e.value.code == -5 and "instance 66: input 3 (element %d) is not below r" % (66 * 5 + 3) in str(e.value)
    assert p.stage_times() == times                     # the device form, which resets them, was never entered
    # the same rows given in DEVICE memory are the kernel's to judge: code 1 with the input's index, -7, the others complete
    dev = torch.tensor(list(b"".join(int(v).to_bytes(32, "little") for r in rows for v in r)), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(zkr_hip.ZkrError) as e:
        p.witness_batch_device(dev)
    assert e.value.code == -7 and "instance 66 input 3 is not below r" in str(e.value)
    assert [j for j, r in enumerate(e.value.reports) if r[0]] == [66, 68] and e.value.reports[66] == (1, 3) and e.value.reports[68] == (1, 0)
    got = p.last
    assert bool((got[66] == 0).all()) and bool((got[68] == 0).all())
    keep = [j for j in range(70) if j not in (66, 68)]
    assert torch.equal(got[keep], before[keep])


def test_inputs_written_on_a_side_stream_are_waited_for(cases, progs):
    """The inputs reach their buffer by a torch copy queued on a side stream behind a long-running fill; the call is given that
    stream and must start after it."""
    import torch
    c, p = cases[2], progs[2]
    n = 65
    host = torch.tensor(list(b"".join(int(v).to_bytes(32, "little") for r in c["rows"][:n] for v in r)), dtype=torch.uint8).pin_memory()
    side = torch.cuda.Stream(device=0)
    buf = torch.zeros(n * 5 * 32, dtype=torch.uint8, device="cuda:0")
    ballast = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(12):
            ballast.fill_(1)              # a few milliseconds: keeps the side stream busy while the call is made
        buf.copy_(host, non_blocking=True)
    out = p.witness_batch_device(buf, stream=side)
    assert _rows_bytes(out) == c["want"][:n]
    side.synchronize()


def _tree(depth, leaves):
    import rollup as o
    t = o.Tree(depth)
    for i, v in leaves.items():
        t.update(i, v)
    return t


def _end_to_end(circuit, rows, public_of, altered_word):
    import torch
    import zkr_hip
    key, vkb = zkr_hip.ProvingKey.setup_r1cs(circuit.r1cs(), toxic=[11, 12, 13, 14, 15])
    cs = zkr_hip.ConstraintSystem.load(circuit.r1cs())
    vk = zkr_hip.VerifyingKey(vkb)
    prog = zkr_hip.WitnessProgram(circuit.program(), statements=circuit.statements)
    try:
        assert key.info()["nVars"] == circuit.n_vars == prog.info()["nVars"] and key.info()["nPublic"] == circuit.n_public == prog.info()["nPublic"]
        wit = prog.witness_batch_device(rows)
        ptrs = [wit[j].data_ptr() for j in range(len(rows))]
        ok, reports = cs.check_device(ptrs)
        assert ok and all(r == {"violated": 0, "first": None, "one_ok": True} for r in reports)
        proofs = key.prove_batch_device(ptrs, rs=list(range(3, 3 + len(rows))), ss=list(range(40, 40 + len(rows))))
        assert vk.verify_each_device(proofs, ptrs) == [0] * len(rows) and vk.all_valid
        host = [_ints(b) for b in _rows_bytes(wit)]
        for j, row in enumerate(rows):
            assert host[j][0] == 1 and host[j][1:1 + circuit.n_public] == public_of(row)
        # one word of one witness altered where it lies: the check names the constraint that binds it, the LAST one
        word = wit[2].view(torch.int64)
        word[4 * altered_word] += 1
        torch.cuda.synchronize()
        ok, reports = cs.check_device(ptrs)
        assert not ok and [j for j, r in enumerate(reports) if r["violated"]] == [2]
        assert reports[2]["first"] == len(circuit.constraints) - 1
    finally:
        for h in (prog, vk, cs, key):
            h.close()


def test_hasher_end_to_end():
    import rollup as o
    from zkr_hip import circuit as C
    rows = [[0, 0], [1, 0], [R - 1, 0], [123456789, 5], [2 ** 200 + 17, R - 1]]
    _end_to_end(C.Hasher(1), rows, lambda row: [o.multi_hash(row[:1], row[1])] + row, altered_word=1)


def test_merkle_leaf_exists_end_to_end():
    from zkr_hip import circuit as C
    t = _tree(2, {0: 5, 1: 6, 2: 7, 3: 8})
    rows = [[5 + i, t.root] + t.path(i) + [i & 1, i >> 1] for i in range(4)] + [[7, t.root] + t.path(2) + [0, 1]]
    _end_to_end(C.MerkleTreeLeafExists(2), rows, lambda row: row[:2], altered_word=2)


def test_leaf_exists_with_a_wrong_leaf_fails_with_the_builders_text():
    import zkr_hip
    from zkr_hip import circuit as C
    c = C.MerkleTreeLeafExists(2)
    t = _tree(2, {3: 99})
    prog = zkr_hip.WitnessProgram(c.program(), statements=c.statements)
    try:
        with pytest.raises(zkr_hip.ZkrError) as e:
            prog.witness_batch_device([[99, t.root] + t.path(3) + [1, 1], [98, t.root] + t.path(3) + [1, 1]])
        assert e.value.code == -7 and "instance 1 violates: the leaf is in the tree with this root" in str(e.value)
    finally:
        prog.close()


def test_info_grows_with_the_piece_and_handles_do_not_leak(cases):
    import torch
    import zkr_hip
    blob = cases[1]["blob"]
    shape = zkr_hip.wprog_shape(blob)
    sizes = {}
    for piece in (64, 4096):
        p = zkr_hip.WitnessProgram(blob, piece=piece)
        sizes[piece] = p.info()["workspaceBytes"]
        assert sizes[piece] == shape["nWires"] * piece * 32 + piece * 8 and p.info()["nWires"] == shape["nWires"]
        p.close()
        p.close()                                              # a second close frees nothing twice
    assert sizes[4096] == 64 * sizes[64]

    def one_round():                                           # 4096 instances x ~300 wires x 32 B = 37 MiB a handle
        for _ in range(2):
            p = zkr_hip.WitnessProgram(blob, piece=4096)
            p.witness_batch_device(cases[1]["rows"][:3])
            p.close()
    one_round()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(5):
        one_round()
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info(0)[0] <= 8 << 20
