"""GPU: the operator's ledger (include/zkr.h zkr_ledger_*, zkr_eddsa_verify_batch, zkr_rollup_witness_batch_from_device;
csrc/zkr_sequencer.hip) against the rule list applied one transaction at a time in Python (tests/sequencer_model.py over
oracle/rollup.py: verify, Tree, leaf_hash and the state transition of process_tx_inputs).  Statuses, the input signals of
every batch byte for byte, the ledger's root, records and paths afterwards; and one chain from a queue of signed transactions
to verified proofs without the inputs or the witnesses leaving the device."""
import ctypes

import pytest

import rollup as o
from sequencer_model import NOT_REACHED, Model, keypair, le, signed_row, sig_ok_oracle

pytestmark = pytest.mark.gpu


def _pair(depth, n_accounts, balance=1000):
    """A ledger on the device and the model beside it, with the same deposits."""
    from zkr_hip import rollup as n
    ledger, model = n.Ledger(depth), Model(depth)
    rows = [(i, keypair(i)[1], balance, 0) for i in range(n_accounts)]
    ledger.deposit(rows)
    for r in rows:
        model.deposit(*r)
    return ledger, model


def _same_state(ledger, model):
    assert ledger.root == model.tree.root
    assert ledger.info()["accounts"] == len(model.accounts)
    for i in range(len(model.accounts)):
        rec, path = ledger.account(i)
        assert rec == model.accounts[i], i
        assert path == model.tree.path(i), i


def _sequence_both(ledger, model, rows, batch):
    status, inputs, consumed = ledger.sequence(rows, batch)
    want_status, want_inputs, want_consumed, _ = model.sequence(rows, batch)
    assert status == want_status and consumed == want_consumed
    assert tuple(inputs.shape) == (len(want_inputs), batch * (18 + 3 * ledger.depth) * 32) and inputs.is_cuda
    host = inputs.cpu().numpy()
    for b, want in enumerate(want_inputs):
        assert host[b].tobytes() == le(want), "batch %d" % b
    _same_state(ledger, model)
    return status, inputs, want_inputs


class _Queue:
    """Rows whose nonces follow the transactions the builder expects to be accepted."""

    def __init__(self, n_accounts):
        self.nonce, self.rows = [0] * n_accounts, []

    def tx(self, frm, to, amount=10, fee=1, accepted=True, **kw):
        nonce = self.nonce[frm] + 1 if frm < len(self.nonce) else 1
        self.rows.append(signed_row(frm, to, amount, fee, nonce, **kw))
        if accepted:
            self.nonce[frm] += 1


def test_verify_batch_equals_the_host_verify_one_by_one():
    from zkr_hip import rollup as n
    msgs, sigs, pubs, want = [], [], [], []

    def case(msg, sig, pub, expect):
        msgs.append(msg), sigs.append(sig), pubs.append(pub), want.append(expect)
    base = []
    for j in range(8):
        priv, pub = keypair(j % 6)
        msg = [j, (j + 1) % 6, 100 + j, 1 + j, 1 + j]
        base.append((msg, n.sign(priv, msg), pub))
    for msg, sig, pub in base:
        case(msg, sig, pub, True)
    flip = lambda v, bit: v ^ (1 << bit)
    for j, (msg, sig, pub) in enumerate(base):
        r8, s = sig["R8"], sig["S"]
        case(msg, {"R8": (flip(r8[0], j), r8[1]), "S": s}, pub, False)          # a flipped bit in R8x (lands off the curve)
        case(msg, {"R8": (r8[0], flip(r8[1], 3 * j)), "S": s}, pub, False)      # ... in R8y
        case(msg, {"R8": r8, "S": flip(s, 31 * j)}, pub, False)                 # ... in S
        case(msg, {"R8": r8, "S": s + o.SUBORDER}, pub, False)                  # S + suborder: the same point, refused by range
        case(msg[:4] + [msg[4] + 1], sig, pub, False)                           # another message
        case(msg, sig, base[(j + 1) % 8][2] if base[(j + 1) % 8][2] != pub else base[(j + 2) % 8][2], False)  # another key
    msg, sig, pub = base[0]
    case(msg, {"R8": (sig["R8"][0], (sig["R8"][1] + 1) % o.R), "S": sig["S"]}, pub, False)      # R8 off the curve
    case(msg, sig, (pub[0], (pub[1] + 1) % o.R), False)                                          # a key off the curve
    case(msg, sig, (0, 1), False)                                                                # the identity as the key
    case(msg, {"R8": (sig["R8"][0] + o.R, sig["R8"][1]), "S": sig["S"]}, pub, False)             # R8x not below r
    case(msg, sig, (pub[0], pub[1] + o.R), False)                                                # a key coordinate not below r
    # the identity as the key under a signature made for it: S * BASE8 == R8 + h * 8 * O for R8 = S * BASE8, any message --
    # verify (crypto.ts:170-177) has no order check, so this holds; the ledger's rule 10 refuses it (test below)
    forged = {"R8": o.bj_mul(o.BASE8, 5), "S": 5}
    case(msg, forged, (0, 1), True)
    case([v + o.R if i == 2 else v for i, v in enumerate(msg)], sig, pub, True)                  # a message element >= r: taken mod r
    case([o.R - 1, 0, (1 << 256) - 1, 5, 6], sig, pub, False)
    while len(msgs) < 64:
        case(*base[len(msgs) % 8], True)
    assert len(msgs) == 64
    got = n.verify_batch(msgs, sigs, pubs)
    # zkr_eddsa_verify refuses a message element that is not below r; multi_hash (host) takes it mod r, and so does the batch
    host = [n.verify([v % o.R for v in m], s, p) for m, s, p in zip(msgs, sigs, pubs)]
    assert got == host
    assert got == want
    assert n.verify_batch([], [], []) == []


def test_sequencing_a_mixed_queue_at_depth_3_batch_2():
    """6 accounts, 16 transactions: the same sender twice in a row, sibling leaves in consecutive transactions, from == to, a
    recipient that is the previous sender, leaves 6 and 7 never touched, three rejected transactions (a bad signature in the middle
    whose nonce the next transaction of that sender reuses), and a 13th accepted transaction that fills no batch."""
    ledger, model = _pair(3, 6)
    q = _Queue(6)
    q.tx(0, 1), q.tx(0, 2)                        # the same sender twice in a row
    q.tx(2, 3), q.tx(3, 2)                        # siblings; the recipient is the previous sender
    q.tx(4, 4)                                    # from == to
    q.tx(1, 0, accepted=False, signer=2)          # signed with another account's key: rule 10
    q.tx(5, 4), q.tx(1, 0)                        # ... and account 1 uses that nonce after all
    q.tx(0, 7, accepted=False)                    # no such recipient: rule 2
    q.tx(2, 2)
    q.tx(3, 1, amount=5000, accepted=False)       # rule 6
    q.tx(4, 5), q.tx(5, 4), q.tx(0, 5), q.tx(1, 3), q.tx(2, 0)
    assert len(q.rows) == 16
    status, inputs, want_inputs = _sequence_both(ledger, model, q.rows, 2)
    assert status == [0, 0, 0, 0, 0, 10, 0, 0, 2, 0, 6, 0, 0, 0, 0, NOT_REACHED]
    assert len(want_inputs) == 6 and ledger.info() == {"depth": 3, "accounts": 6, "applied": 12, "batches": 6}
    # what was not reached is decided by the next call
    status2, _, _ = _sequence_both(ledger, model, q.rows[15:] + [signed_row(3, 3, 1, 1, model.accounts[3][3] + 1)], 2)
    assert status2 == [0, 0]


def test_depth_1_batch_1():
    """Two accounts: the sibling of either leaf is always the other account."""
    ledger, model = _pair(1, 2)
    q = _Queue(2)
    q.tx(0, 1), q.tx(1, 0), q.tx(0, 0), q.tx(1, 1), q.tx(1, 1), q.tx(0, 1)
    status, _, want_inputs = _sequence_both(ledger, model, q.rows, 1)
    assert status == [0] * 6 and len(want_inputs) == 6


def test_two_calls_with_a_deposit_between_them_equal_one_model_run():
    """The second call's -1 source is what the first call and the deposit stored."""
    ledger, model = _pair(3, 4)
    q = _Queue(5)
    q.tx(0, 1), q.tx(1, 2), q.tx(2, 3), q.tx(3, 0)
    first = _sequence_both(ledger, model, q.rows, 2)
    assert first[0] == [0] * 4
    for row in ((4, keypair(4)[1], 500, 0), (1, keypair(1)[1], 77, model.accounts[1][3])):      # a new account; an overwritten balance
        ledger.deposit(*row)
        model.deposit(*row)
    _same_state(ledger, model)
    q.rows = []
    q.tx(4, 1), q.tx(1, 4), q.tx(0, 4), q.tx(2, 2)
    second = _sequence_both(ledger, model, q.rows, 2)
    assert second[0] == [0] * 4 and ledger.info()["applied"] == 8 and ledger.info()["batches"] == 4


def test_a_small_order_key_fails_rule_10():
    """verify (crypto.ts) accepts a signature made for the identity key; the circuit does not, and neither does the ledger."""
    from zkr_hip import rollup as n
    ledger, model = n.Ledger(2), Model(2)
    for row in ((0, (0, 1), 1000, 0), (1, keypair(1)[1], 1000, 0)):
        ledger.deposit(*row)
        model.deposit(*row)
    forged = n.tx_row(0, 1, 10, 1, 1, {"R8": o.bj_mul(o.BASE8, 5), "S": 5})
    assert o.verify(forged[:5], tuple(forged[5:]), (0, 1)) and not sig_ok_oracle(forged, (0, 1))
    status, _, _ = _sequence_both(ledger, model, [forged, signed_row(1, 0, 10, 1, 1)], 1)
    assert status == [10, 0]


def test_a_queue_with_no_accepted_transaction():
    ledger, model = _pair(2, 3)
    root = ledger.root
    rows = [signed_row(0, 1, 10, 1, 5), signed_row(1, 2, 0, 1, 1), signed_row(2, 9, 1, 1, 1)]
    status, inputs, want_inputs = _sequence_both(ledger, model, rows, 1)
    assert status == [NOT_REACHED] * 3 and want_inputs == [] and inputs.shape[0] == 0
    assert ledger.root == root and ledger.info()["applied"] == 0 and ledger.info()["batches"] == 0
    assert ledger.sequence([], 2)[0] == []
    # one accepted transaction fills no batch of two either
    status, inputs, consumed = ledger.sequence([signed_row(0, 1, 10, 1, 1)], 2)
    assert status == [NOT_REACHED] and inputs.shape[0] == 0 and consumed == 0 and ledger.root == root


def test_an_error_leaves_the_ledger_unchanged():
    import zkr_hip
    ledger, model = _pair(2, 3)
    L = zkr_hip.lib()
    rows = [signed_row(0, 1, 10, 1, 1), signed_row(1, 2, 10, 1, 1)]
    buf, status = le(v for r in rows for v in r), ctypes.create_string_buffer(2)
    nb, consumed = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.zkr_ledger_sequence(ledger._h, buf, 2, 1, status, None, ctypes.byref(nb), ctypes.byref(consumed), None) == -5
    assert b"null" in L.zkr_last_error()
    import torch
    room = torch.empty(2 * 24 * 32, dtype=torch.uint8, device="cuda")
    assert L.zkr_ledger_sequence(ledger._h, buf, 2, 0, status, room.data_ptr(), ctypes.byref(nb), ctypes.byref(consumed), None) == -5   # batch 0
    assert L.zkr_ledger_sequence(None, buf, 2, 1, status, room.data_ptr(), ctypes.byref(nb), ctypes.byref(consumed), None) == -5
    _same_state(ledger, model)
    assert ledger.info()["applied"] == 0
    assert _sequence_both(ledger, model, rows, 1)[0] == [0, 0]


def test_deposit_inserts_overwrites_and_refuses_an_index_out_of_sync():
    import zkr_hip
    from zkr_hip import rollup as n
    depth = 4
    ledger = n.Ledger(depth)
    empty = n.BalanceTree.from_leaves(depth, [])
    assert ledger.root == empty.root == o.Tree(depth).root and ledger.info() == {"depth": 4, "accounts": 0, "applied": 0, "batches": 0}
    recs = [[keypair(i)[1][0], keypair(i)[1][1], 100 + i, i] for i in range(5)]
    ledger.deposit([(i, r[:2], r[2], r[3]) for i, r in enumerate(recs[:3])])                     # three inserts in one call
    ledger.deposit(3, recs[3][:2], recs[3][2], recs[3][3])
    recs[1][2] = 999
    ledger.deposit([(1, recs[1][:2], 999, recs[1][3]), (4, recs[4][:2], recs[4][2], recs[4][3]), (4, recs[4][:2], 5, 6)])   # overwrite, insert, overwrite what was just inserted
    recs[4][2:] = [5, 6]
    want = n.BalanceTree.from_leaves(depth, [o.leaf_hash(r[:2], r[2], r[3]) for r in recs])
    assert ledger.root == want.root
    for i, r in enumerate(recs):
        assert ledger.account(i) == (r, want.path(i))
    for bad, why in (([(6, recs[0][:2], 1, 0)], "out of sync"), ([(5, recs[0][:2], 1, 0), (7, recs[0][:2], 1, 0)], "out of sync"),
                     ([(0, (o.R, 1), 1, 0)], "not below r"), ([(0, recs[0][:2], 1 << 250, 0)], "250 bits")):
        with pytest.raises(zkr_hip.ZkrError) as e:
            ledger.deposit(bad)
        assert e.value.code == -5 and why in str(e.value)
    assert ledger.root == want.root and ledger.info()["accounts"] == 5                           # a refused call changes nothing
    with pytest.raises(zkr_hip.ZkrError):
        ledger.account(5)
    full = n.Ledger(1)
    full.deposit([(0, recs[0][:2], 1, 0), (1, recs[1][:2], 1, 0)])
    with pytest.raises(zkr_hip.ZkrError):
        full.deposit(2, recs[2][:2], 1, 0)


def test_from_a_queue_to_verified_proofs_on_the_device():
    """setup_r1cs -> sequence of 8 transactions -> calculate_witness_batch_from_device -> r1cs check -> prove_batch_device ->
    verify_each_device for RollupCircuit(2, 3): every system satisfied, every verdict "valid", and the witnesses are the bytes
    calculate_witness_batch_device builds from the same inputs passed from the host."""
    import torch
    import zkr_hip
    from zkr_hip import rollup as n
    c = n.RollupCircuit(2, 3)
    r1cs = c.r1cs()
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=[2, 3, 5, 7, 11])
    cs = zkr_hip.ConstraintSystem.load(r1cs)
    ledger, model = _pair(3, 5)
    q = _Queue(5)
    q.tx(0, 1), q.tx(1, 0), q.tx(2, 2), q.tx(3, 4), q.tx(4, 3), q.tx(0, 4), q.tx(0, 2), q.tx(3, 2)
    status, inputs, want_inputs = _sequence_both(ledger, model, q.rows, 2)
    assert status == [0] * 8 and inputs.shape[0] == 4
    stream = torch.cuda.current_stream().cuda_stream
    wit = c.calculate_witness_batch_from_device(inputs, stream=stream)
    ptrs = [wit[i].data_ptr() for i in range(4)]
    ok, reports = cs.check_device(ptrs, stream=stream)
    assert ok is True and all(r["violated"] == 0 for r in reports)
    proofs = key.prove_batch_device(ptrs, [5, 6, 7, 8], [9, 10, 11, 12])
    with zkr_hip.VerifyingKey(vk_bin) as vk:
        assert vk.verify_each_device(proofs, ptrs) == [0, 0, 0, 0] and vk.all_valid
    from_host = c.calculate_witness_batch_device(want_inputs)
    assert torch.equal(wit, from_host)
    assert c.public_signals(bytes(wit[3].cpu().numpy().tobytes()))[0] == ledger.root
    # the second entry refuses what the first refuses: inputs that do not satisfy the circuit, and a tensor of another shape
    stale = inputs.clone()
    stale[1, :32] = inputs[0, :32]                                      # batch 1 starts from batch 0's root
    with pytest.raises(zkr_hip.ZkrError) as e:
        c.calculate_witness_batch_from_device(stale)
    assert e.value.code == -7 and "batch 1" in str(e.value)
    with pytest.raises(zkr_hip.ZkrError):
        c.calculate_witness_batch_from_device(inputs[:, :-32])
    cs.close()
