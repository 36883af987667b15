"""GPU: keeping the ledger (include/zkr.h zkr_ledger_records .. zkr_ledger_audit; csrc/zkr_sequencer.hip) against the
models of the sequencer and replay tests (tests/sequencer_model.py, tests/replay_model.py over oracle/rollup.py): read-out,
snapshot -> bulk restore round trips, refusals by the rebuilt root, checkpoints and rollback, the audit, and a restored ledger
that follows the chain.  Wherever a state is compared, the whole stored tree is compared byte for byte with the model's levels,
not only the paths."""
import copy
import ctypes
import functools
import os

import pytest

import rollup as o
from replay_model import n_public, publish, replay
from sequencer_model import NOT_REACHED, Model, keypair, le, sig_ok_oracle, signed_row
from test_gpu_sequencer import _pair, _Queue
from test_ledger_state_cpu import build_blob

pytestmark = pytest.mark.gpu

BATCH = 2


@functools.lru_cache(maxsize=None)
def _sig_ok_cached(row, pub):
    return sig_ok_oracle(list(row), list(pub))


def _sig_ok(row, pub):
    return _sig_ok_cached(tuple(row), tuple(pub))


def _level_offset(depth, l):
    return (2 << depth) - (2 << (depth - l))


def _tree_bytes(ledger):
    import torch
    torch.cuda.synchronize()
    return ledger.tree().cpu().numpy().tobytes()


def _model_tree_bytes(model):
    return b"".join(le(level) for level in model.tree.levels)         # leaves first, root last: the stored layout


def _full_state(ledger, model, applied=None, batches=None):
    n = len(model.accounts)
    info = ledger.info()
    assert info["accounts"] == n and info["depth"] == model.depth
    if applied is not None:
        assert (info["applied"], info["batches"]) == (applied, batches)
    assert ledger.root == model.tree.root
    assert ledger.records() == model.records()
    assert _tree_bytes(ledger) == _model_tree_bytes(model)
    assert ledger.paths(range(n)) == [model.tree.path(i) for i in range(n)]
    assert ledger.audit() is None


def _seq_both(ledger, model, rows, batch=BATCH):
    """ledger.sequence against model.sequence: statuses, input bytes, consumed.  -> (status, input bytes, consumed)."""
    status, inputs, consumed = ledger.sequence(rows, batch)
    want_status, want_inputs, want_consumed, _ = model.sequence(rows, batch, sig_ok=_sig_ok)
    got = inputs.cpu().numpy().tobytes()
    assert status == want_status and consumed == want_consumed
    assert got == b"".join(le(w) for w in want_inputs)
    return status, got, consumed


def _queue(model, pairs):
    """Signed rows for (from, to) pairs whose nonces continue the model's."""
    q = _Queue(len(model.accounts))
    q.nonce = [model.accounts[i][3] for i in range(len(model.accounts))]
    for frm, to in pairs:
        q.tx(frm, to)
    return q.rows


def _refused(code, call, word=None):
    import zkr_hip
    with pytest.raises(zkr_hip.ZkrError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    return str(e.value)


# ------------------------------------------------------------------------------------------------ read-out
def test_read_out_after_deposits_and_a_sequence():
    a, m = _pair(3, 6)
    _seq_both(a, m, _queue(m, [(0, 1), (1, 2), (2, 3), (5, 4)]))
    assert a.records() == m.records()
    assert a.records(2, 3) == m.records()[2:5] and a.records(6, 0) == [] and a.records(0, 0) == []
    _refused(-5, lambda: a.records(4, 3), "accounts")
    _refused(-5, lambda: a.records(7, 0))
    view = a.tree()
    assert tuple(view.shape) == (15, 32) and view.is_cuda and str(view.dtype) == "torch.uint8"
    paths = a.paths(range(6))
    assert paths == [a.account(i)[1] for i in range(6)] == [m.tree.path(i) for i in range(6)]
    assert a.paths([7, 0, 7]) == [m.tree.path(7), m.tree.path(0), m.tree.path(7)] and a.paths([]) == []   # any leaf of the tree has a path
    with pytest.raises(ValueError):
        a.paths([8])
    assert _tree_bytes(a) == _model_tree_bytes(m)


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("depth,n", [(3, 0), (3, 1), (3, 2), (3, 3), (3, 5), (3, 8), (5, 5)])
def test_snapshot_restore_round_trip(depth, n, tmp_path):
    from zkr_hip import rollup as nat
    a, m = _pair(depth, n)
    applied = batches = 0
    if n >= 2:                                                        # counters that are not zero
        _seq_both(a, m, _queue(m, [(0, 1), (1, 0)]))
        applied, batches = 2, 1
    blob = a.snapshot()
    assert blob == build_blob(depth, m.records(), applied, batches)  # the writer against the table of include/zkr.h, byte for byte
    assert nat.Ledger.snapshot_check(blob) == ({"depth": depth, "accounts": n, "applied": applied, "batches": batches}, None)
    b = nat.Ledger.restore(blob)
    assert b.depth == depth and b.info() == a.info()
    _full_state(b, m, applied, batches)
    assert b.snapshot() == blob
    assert b.journal_info() == (0, 0)
    # through a file: the same bytes, nothing left beside it; a truncated file is refused
    path = str(tmp_path / "ledger.bin")
    a.save(path)
    a.save(path)                                                      # over an existing file
    assert open(path, "rb").read() == blob and os.listdir(str(tmp_path)) == ["ledger.bin"]
    c = nat.Ledger.load(path)
    _full_state(c, m, applied, batches)
    assert c.snapshot() == blob
    c.close()
    with open(path, "wb") as f:
        f.write(blob[:-1])
    _refused(-5, lambda: nat.Ledger.load(path), "length")
    # fill both to 2^depth: every node no earlier path touched is now under a path
    N = 1 << depth
    more = [(i, keypair(i)[1], 1000, 0) for i in range(n, N)]
    if more:
        a.deposit(more), b.deposit(more)
        for r in more:
            m.deposit(*r)
    _full_state(a, m, applied, batches)
    _full_state(b, m, applied, batches)
    # one queue on the original and on the restored ledger: the same statuses and input bytes
    rows = _queue(m, [(0, N - 1), (N - 1, 2 % N), (1, 0), (n % N, 1)])
    before = copy.deepcopy(m)
    got_a = _seq_both(a, m, rows)
    status_b, inputs_b, consumed_b = b.sequence(rows, BATCH)
    assert (status_b, inputs_b.cpu().numpy().tobytes(), consumed_b) == got_a and got_a[0] == [0] * 4
    assert before.tree.root != m.tree.root
    _full_state(a, m, applied + 4, batches + 2)
    _full_state(b, m, applied + 4, batches + 2)
    assert a.snapshot() == b.snapshot()


def test_bulk_build_past_one_piece_of_records_equals_the_tree_builder():
    """2^20 + 3 accounts at depth 21: the records go up in two pieces, and level l has ceil(accounts / 2^l) populated nodes with
    a spine of single nodes above the three odd ones.  The reference is built by kernels that are not the ledger's: every leaf
    hash by zkr_mimcsponge_multihash_batch, the whole tree by zkr_balance_tree_build; all (2^22 - 1) x 32 B are compared.  The
    audit then finds a leaf of the second piece that was changed, and nothing once it is back."""
    import numpy as np
    import torch
    import zkr_hip
    from zkr_hip import rollup as nat
    depth, n = 21, (1 << 20) + 3
    rng = np.random.default_rng(0x5A4B)
    recs = np.zeros((n, 4, 4), dtype=np.uint64)
    recs[:, :, 0] = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    recs[:, :2, 3] = rng.integers(0, 1 << 60, size=(n, 2), dtype=np.uint64)     # keys up to 2^252 < r, balances and nonces small
    raw = recs.tobytes()
    L = zkr_hip.lib()
    leaves = np.zeros(((1 << depth), 32), dtype=np.uint8)
    out = ctypes.create_string_buffer(32 * n)
    assert L.zkr_mimcsponge_multihash_batch(raw, n, 4, out, 0) == 0
    leaves[:n] = np.frombuffer(out, dtype=np.uint8).reshape(n, 32)
    levels = ctypes.create_string_buffer(32 * ((2 << depth) - 1))
    assert L.zkr_balance_tree_build(leaves.tobytes(), depth, levels, 0) == 0
    want = np.frombuffer(levels, dtype=np.uint8)
    root = int.from_bytes(want[-32:].tobytes(), "little")
    tag = nat.multi_hash([depth, n, 9, 4, root])
    import struct
    blob = b"ZKRLEDG1" + struct.pack("<IIQQQ", depth, 0, n, 9, 4) + bytes(24) + le([root]) + le([tag]) + raw
    a = nat.Ledger.restore(blob)
    assert a.info() == {"depth": depth, "accounts": n, "applied": 9, "batches": 4} and a.root == root
    view = a.tree()
    assert torch.equal(view.view(-1), torch.from_numpy(want.copy()).cuda())
    assert a.audit() is None
    assert a.records(n - 2, 2) == [[int.from_bytes(raw[128 * i + 32 * j:128 * i + 32 * j + 32], "little") for j in range(4)] for i in (n - 2, n - 1)]
    for level, index in ((0, (1 << 20) + 1), (0, 5), (20, 1), (0, n)):   # second piece, first piece, the spine, the first empty leaf
        row = _level_offset(depth, level) + index
        view[row, 0] ^= 1
        torch.cuda.synchronize()
        assert a.audit() == (level, index)
        view[row, 0] ^= 1
    torch.cuda.synchronize()
    assert a.audit() is None


# ------------------------------------------------------------------------------------------------ refusals by the root
def test_a_snapshot_whose_records_do_not_rebuild_to_its_root_is_refused():
    import zkr_hip
    from zkr_hip import rollup as nat
    a, m = _pair(3, 5)
    blob = a.snapshot()
    hexa = lambda v: "0x%064x" % v

    def rebuilt(spoiled):
        t = o.Tree(3)
        for i in range(5):
            r = [int.from_bytes(spoiled[128 + 128 * i + 32 * j:128 + 128 * i + 32 * j + 32], "little") for j in range(4)]
            t.update(i, o.leaf_hash(r[:2], r[2], r[3]))
        return t.root
    at = 128 + 128 * 2 + 64 + 1
    flipped = blob[:at] + bytes([blob[at] ^ 0x04]) + blob[at + 1:]    # one balance bit: the tag does not cover it, the root does
    swapped = blob[:128] + blob[128 + 128:128 + 256] + blob[128:128 + 128] + blob[128 + 256:]
    L = zkr_hip.lib()
    for bad in (flipped, swapped):
        assert nat.Ledger.snapshot_check(bad)[0] is not None         # well-formed: only the rebuild can tell
        msg = _refused(-2, lambda: nat.Ledger.restore(bad))
        assert hexa(m.tree.root) in msg and hexa(rebuilt(bad)) in msg and rebuilt(bad) != m.tree.root
        h = ctypes.c_void_p()
        assert L.zkr_ledger_restore(bad, len(bad), 0, ctypes.byref(h)) == -2 and not h.value
    root_bit = blob[:64 + 3] + bytes([blob[64 + 3] ^ 1]) + blob[64 + 4:]
    _refused(-5, lambda: nat.Ledger.restore(root_bit), "tag")
    h = ctypes.c_void_p()
    assert L.zkr_ledger_restore(root_bit, len(root_bit), 0, ctypes.byref(h)) == -5 and not h.value
    _full_state(nat.Ledger.restore(blob), m, 0, 0)                    # the untouched blob still restores


# ------------------------------------------------------------------------------------------------ rollback
PAIRS_6 = [(0, 1), (1, 2), (2, 3), (3, 2), (4, 4), (5, 4), (1, 0), (2, 2)]


def test_rollback_of_a_sequence_and_the_same_bytes_again():
    a, m = _pair(3, 6)
    rows = _queue(m, PAIRS_6)
    tree0 = _tree_bytes(a)
    assert a.journal_info() == (0, 0)
    cp = a.checkpoint()
    assert a.journal_info() == (1, 0)
    first = a.sequence(rows, BATCH)
    first = (first[0], first[1].cpu().numpy().tobytes(), first[2])
    assert first[0] == [0] * 8 and a.info()["applied"] == 8 and a.journal_info()[1] > 0 and _tree_bytes(a) != tree0
    a.rollback(cp)
    assert _tree_bytes(a) == tree0 and a.journal_info() == (1, 0)
    _full_state(a, m, 0, 0)
    assert _seq_both(a, m, rows) == first                             # and the model agrees with both runs
    _full_state(a, m, 8, 4)
    a.rollback(cp)                                                    # the checkpoint stayed open: once more
    assert _tree_bytes(a) == tree0 and a.info()["applied"] == 0
    a.release(cp)
    assert a.journal_info() == (0, 0)


def test_the_deposit_race():
    """a Deposit event makes the sequenced batches stale.  Roll back, deposit (a top-up of an account that
    sends in the queue, and a new account), sequence the same queue again: the result is that of a ledger that saw the deposit
    first."""
    a, m = _pair(3, 5)
    rows = _queue(m, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2)])
    cp = a.checkpoint()
    stale = a.sequence(rows, BATCH)
    assert stale[0] == [0] * 6
    a.rollback(cp)
    event = [(0, keypair(0)[1], 5000, 0), (5, keypair(5)[1], 700, 0)]
    a.deposit(event)
    for r in event:
        m.deposit(*r)
    fresh = _seq_both(a, m, rows)
    assert fresh[0] == [0] * 6 and fresh[1] != stale[1].cpu().numpy().tobytes()
    _full_state(a, m, 6, 3)
    a.release(cp)
    assert a.journal_info() == (0, 0)
    _full_state(a, m, 6, 3)


def test_rollback_over_inserting_deposits():
    a, m = _pair(3, 3)
    tree0 = _tree_bytes(a)
    cp = a.checkpoint()
    a.deposit([(3, keypair(3)[1], 10, 0), (1, keypair(1)[1], 77, 4), (4, keypair(4)[1], 20, 0), (3, keypair(3)[1], 11, 1)])
    assert a.info()["accounts"] == 5 and a.account(3)[0][2:] == [11, 1]
    a.rollback(cp)
    assert a.info()["accounts"] == 3 and _tree_bytes(a) == tree0
    _full_state(a, m, 0, 0)
    _refused(-5, lambda: a.account(3))
    _refused(-5, lambda: a.records(3, 1))
    a.deposit(3, keypair(9)[1], 55)                                   # the index is free again, for another record
    m.deposit(3, keypair(9)[1], 55)
    _full_state(a, m, 0, 0)


def test_nested_checkpoints():
    a, m0 = _pair(3, 4)
    cp1 = a.checkpoint()
    new = (4, keypair(4)[1], 300, 0)
    a.deposit(*new)
    m1 = copy.deepcopy(m0)
    m1.deposit(*new)
    cp2 = a.checkpoint()
    assert cp2 > cp1 and a.journal_info()[0] == 2
    rows = _queue(m1, [(4, 0), (0, 4), (1, 2), (2, 1)])
    assert a.sequence(rows, BATCH)[0] == [0] * 4
    a.rollback(cp2)
    _full_state(a, m1, 0, 0)
    assert a.journal_info()[0] == 2
    a.rollback(cp1)
    _full_state(a, m0, 0, 0)
    assert a.journal_info() == (1, 0)                                 # cp2 was taken after cp1: it went with the rollback
    _refused(-5, lambda: a.rollback(cp2), "checkpoint")
    # straight over both
    a.deposit(*new)
    cp3 = a.checkpoint()
    assert cp3 > cp2
    assert a.sequence(rows, BATCH)[0] == [0] * 4 and a.info() == {"depth": 3, "accounts": 5, "applied": 4, "batches": 2}
    a.rollback(cp1)
    _full_state(a, m0, 0, 0)
    _refused(-5, lambda: a.rollback(cp3), "checkpoint")
    _refused(-5, lambda: a.release(cp3), "checkpoint")
    assert a.journal_info() == (1, 0)
    # a released inner checkpoint leaves the outer one whole
    a.deposit(*new)
    cp4 = a.checkpoint()
    assert a.sequence(rows, BATCH)[0] == [0] * 4
    a.release(cp4)
    assert a.journal_info()[0] == 1 and a.info()["applied"] == 4
    a.rollback(cp1)
    _full_state(a, m0, 0, 0)


def test_three_calls_over_the_same_nodes_under_one_checkpoint():
    """Two sequences over the same leaves, then a replay whose middle batch is refused -- the truncated store of
    tests/test_gpu_replay.py, where the stored list is a prefix of the hashed one.  Every call journals the nodes it overwrites,
    the same nodes three times; the undo runs call by call, the latest first, and the whole tree view ends byte-identical to the
    copy taken at the checkpoint."""
    a, m = _pair(3, 6)
    start = copy.deepcopy(m)
    tree0, records0 = _tree_bytes(a), a.records()
    cp = a.checkpoint()
    _seq_both(a, m, _queue(m, [(0, 1), (1, 2), (2, 3), (3, 0)]))
    nodes1 = a.journal_info()[1]
    _seq_both(a, m, _queue(m, [(1, 0), (0, 3), (3, 2), (2, 1)]))
    nodes2 = a.journal_info()[1]
    assert 0 < nodes1 < nodes2
    ahead = copy.deepcopy(m)
    publics = publish(ahead, _queue(m, [(0, 1), (1, 0), (2, 3), (3, 2), (0, 1), (2, 3)]), BATCH)   # batches 0 and 2 write leaves 0 and 1
    spoiled = [list(p) for p in publics]
    at = n_public(BATCH, 3) - 1                                       # the last intermediate path element of batch 1
    spoiled[1][at] = (spoiled[1][at] + 1) % o.R
    want = ([0, 4, NOT_REACHED], [0, at, 0], 1)
    assert replay(m, spoiled, BATCH) == want                          # the model moves over batch 0 alone
    assert a.replay(spoiled, BATCH) == want
    _full_state(a, m, 10, 5)
    assert a.journal_info()[1] > nodes2
    a.rollback(cp)
    assert _tree_bytes(a) == tree0 and a.records() == records0
    _full_state(a, start, 0, 0)
    assert a.journal_info() == (1, 0)


def test_release_forgets_the_checkpoint_and_the_ledger_keeps_working():
    a, m = _pair(3, 4)
    cp = a.checkpoint()
    top_up = (2, keypair(2)[1], 4321, 0)
    a.deposit(*top_up)
    m.deposit(*top_up)
    assert a.journal_info() == (1, 4)                                 # a leaf, two inner nodes, the root
    a.release(cp)
    assert a.journal_info() == (0, 0)
    _refused(-5, lambda: a.rollback(cp), "checkpoint")
    _refused(-5, lambda: a.release(cp), "checkpoint")
    _refused(-5, lambda: a.rollback(12345), "checkpoint")
    _full_state(a, m, 0, 0)
    _seq_both(a, m, _queue(m, [(2, 3), (3, 2)]))
    assert a.journal_info() == (0, 0)                                 # nothing more is recorded
    _full_state(a, m, 2, 1)


def test_a_refused_call_under_a_checkpoint_leaves_the_journal_as_it_was():
    a, m = _pair(3, 4)
    start = copy.deepcopy(m)
    cp = a.checkpoint()
    top_up = (1, keypair(1)[1], 999, 0)
    a.deposit(*top_up)
    m.deposit(*top_up)
    journal = a.journal_info()
    assert journal == (1, 4)
    _refused(-5, lambda: a.deposit(6, keypair(6)[1], 5), "out of sync")
    _refused(-5, lambda: a.deposit([(4, keypair(4)[1], 5, 0), (1, keypair(1)[1], 1 << 250, 0)]))   # refused as a whole
    rows = _queue(m, [(0, 1), (1, 0)])
    _refused(-5, lambda: a.sequence(rows, 5000), "batch")            # a geometry zkr_rollup_info refuses
    _refused(-5, lambda: a.replay(b"", 5000), "batch")
    assert a.journal_info() == journal
    _full_state(a, m, 0, 0)
    a.rollback(cp)
    _full_state(a, start, 0, 0)


# ------------------------------------------------------------------------------------------------ audit
def test_audit_is_sound_on_every_shape_of_ledger():
    from zkr_hip import rollup as nat
    assert nat.Ledger(3).audit() is None and nat.Ledger(1).audit() is None
    for depth, n in ((3, 5), (3, 8), (5, 5), (1, 1), (4, 9)):
        a, m = _pair(depth, n)
        assert a.audit() is None
    a, m = _pair(3, 6)
    cp = a.checkpoint()
    _seq_both(a, m, _queue(m, [(0, 1), (1, 2), (5, 4), (4, 5)]))
    assert a.audit() is None
    a.rollback(cp)
    assert a.audit() is None


def test_audit_names_the_node_that_was_changed():
    """One stored node XOR 1 in its lowest byte, through the tree view, and back after each case.  This only changes data that
    the kernels hash and compare; no index or pointer is derived from it."""
    import torch
    import zkr_hip
    a, m = _pair(3, 5)
    view = a.tree()
    row = lambda level, index: _level_offset(3, level) + index

    def flip(level, index):
        view[row(level, index), 0] ^= 1
        torch.cuda.synchronize()
    # a populated leaf, an empty leaf, an inner node above accounts, an inner node in the empty region, the root
    for target in ((0, 2), (0, 6), (1, 1), (1, 3), (3, 0), (0, 4), (0, 5), (1, 2), (2, 1)):
        flip(*target)
        assert a.audit() == target
        assert b"audit" in zkr_hip.lib().zkr_last_error()
        flip(*target)
        assert a.audit() is None
    flip(2, 1), flip(1, 0)                                            # two bad nodes: the lower level wins
    assert a.audit() == (1, 0)
    flip(1, 3)                                                        # ... then the lower index
    assert a.audit() == (1, 0)
    flip(1, 0)
    assert a.audit() == (1, 3)
    flip(1, 3)
    assert a.audit() == (2, 1)
    flip(2, 1)
    assert a.audit() is None
    _full_state(a, m, 0, 0)


# ------------------------------------------------------------------------------------------------ chain
def test_a_restored_ledger_follows_the_chain():
    from zkr_hip import rollup as nat
    a, m = _pair(3, 6)
    _seq_both(a, m, _queue(m, [(0, 1), (1, 2), (2, 3), (3, 0)]))
    b = nat.Ledger.restore(a.snapshot())
    rows = _queue(m, [(4, 5), (5, 4), (0, 5), (1, 1)])
    publics = publish(m, rows, BATCH)                                 # what the operator publishes next; m moves along
    assert b.replay(publics, BATCH, signatures=True) == ([0, 0], [0, 0], 2)
    assert b.info() == {"depth": 3, "accounts": 6, "applied": 4 + len(rows), "batches": 4}
    _full_state(b, m, 8, 4)
