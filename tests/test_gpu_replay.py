"""GPU: following the chain (include/zkr.h zkr_ledger_replay, zkr_ledger_replay_device; csrc/zkr_sequencer.hip) against
tests/replay_model.py, which applies a published batch one transaction at a time over oracle/rollup.py and derives its full
public signal list again.  One ledger sequences a queue, a second one with the same deposits replays what the first published:
verdicts, `where`, and the second ledger's root, records and paths afterwards -- after a clean run, after a refusal at every
signal of a batch, after a refusal in the middle of a run, and once through real proofs."""
import copy
import ctypes
import functools

import pytest

import rollup as o
from replay_model import judge, n_public, publish, replay, tx_base
from sequencer_model import NOT_REACHED, Model, keypair, le, sig_ok_oracle, signed_row
from test_gpu_sequencer import _pair, _Queue, _same_state

pytestmark = pytest.mark.gpu

DEPTH, BATCH = 3, 2
NP = n_public(BATCH, DEPTH)


@functools.lru_cache(maxsize=None)
def _sig_ok_cached(row, pub):
    return sig_ok_oracle(list(row), list(pub))


def _sig_ok(row, pub):
    return _sig_ok_cached(tuple(row), tuple(pub))


def _witnesses(publics):
    """Plain tensors standing in for witnesses: words 1..n_public hold the signals, every other word is noise."""
    import torch
    width = len(publics[0])
    w = torch.full((len(publics), (width + 3) * 32), 0xA5, dtype=torch.uint8, device="cuda")
    for b, p in enumerate(publics):
        w[b, 32:32 * (1 + width)] = torch.frombuffer(bytearray(le(p)), dtype=torch.uint8).cuda()
    return w, [w[b].data_ptr() for b in range(len(publics))]


def _replay(ledger, form, publics, batch, **kw):
    if form == "host":
        return ledger.replay(publics, batch, **kw)
    w, ptrs = _witnesses(publics)
    return ledger.replay_device(ptrs, batch, **kw)


def _mixed_rows():
    """The queue of test_sequencing_a_mixed_queue_at_depth_3_batch_2: 16 transactions, 12 of them applied."""
    q = _Queue(6)
    q.tx(0, 1), q.tx(0, 2), q.tx(2, 3), q.tx(3, 2), q.tx(4, 4)
    q.tx(1, 0, accepted=False, signer=2)
    q.tx(5, 4), q.tx(1, 0)
    q.tx(0, 7, accepted=False)
    q.tx(2, 2)
    q.tx(3, 1, amount=5000, accepted=False)
    q.tx(4, 5), q.tx(5, 4), q.tx(0, 5), q.tx(1, 3), q.tx(2, 0)
    return q.rows


@pytest.fixture(scope="module")
def chain():
    """Ledger A has sequenced the mixed queue; `publics` is what it published: its input rows with the model's new roots in
    front.  `start` is the model after the deposits, `states[b]` the model after b batches."""
    a, start = _pair(DEPTH, 6)
    rows = _mixed_rows()
    status, inputs, consumed = a.sequence(rows, BATCH)
    assert consumed == 15 and inputs.shape[0] == 6
    applied = [r for r, s in zip(rows, status) if s == 0]
    assert len(applied) == 12
    m, states, want = copy.deepcopy(start), [copy.deepcopy(start)], []
    for b in range(6):
        want += publish(m, applied[2 * b:2 * b + 2], BATCH)
        states.append(copy.deepcopy(m))
    host = inputs.cpu().numpy()
    publics = [[want[b][0]] + [int.from_bytes(host[b, i:i + 32].tobytes(), "little") for i in range(0, host.shape[1], 32)] for b in range(6)]
    assert publics == want                                            # A's rows are the model's batch_public_signals
    _same_state(a, m)
    return {"a": a, "start": start, "states": states, "publics": publics}


@pytest.mark.parametrize("form", ["host", "device"])
def test_round_trip_without_proofs(chain, form):
    b, _ = _pair(DEPTH, 6)
    verdicts, where, applied = _replay(b, form, chain["publics"], BATCH)
    assert verdicts == [0] * 6 and where == [0] * 6 and applied == 6
    assert b.root == chain["a"].root
    _same_state(b, chain["states"][6])
    assert b.info() == {"depth": 3, "accounts": 6, "applied": 12, "batches": 6}
    # the same with the signatures looked at, one batch per call
    c, _ = _pair(DEPTH, 6)
    for p in chain["publics"]:
        assert _replay(c, form, [p], BATCH, signatures=True) == ([0], [0], 1)
    _same_state(c, chain["states"][6])
    assert replay(copy.deepcopy(chain["start"]), chain["publics"], BATCH, signatures=True, sig_ok=_sig_ok) == ([0] * 6, [0] * 6, 6)


@pytest.mark.parametrize("form", ["host", "device"])
def test_depth_1_batch_1(form):
    a, start = _pair(1, 2)
    q = _Queue(2)
    q.tx(0, 1), q.tx(1, 0), q.tx(0, 0), q.tx(1, 1), q.tx(1, 1), q.tx(0, 1)
    m = copy.deepcopy(start)
    publics = publish(m, q.rows, 1)
    status, inputs, _ = a.sequence(q.rows, 1)
    assert status == [0] * 6 and inputs.cpu().numpy().tobytes() == b"".join(le(p[1:]) for p in publics)
    b, _ = _pair(1, 2)
    assert _replay(b, form, publics, 1, signatures=True) == ([0] * 6, [0] * 6, 6)
    _same_state(b, m)
    assert b.root == a.root
    spoiled = [list(p) for p in publics]
    spoiled[4][n_public(1, 1) - 1] ^= 1                               # the last path element of the fifth batch
    c, _ = _pair(1, 2)
    assert _replay(c, form, spoiled, 1) == ([0, 0, 0, 0, 4, NOT_REACHED], [0, 0, 0, 0, n_public(1, 1) - 1, 0], 4)
    want = copy.deepcopy(start)
    assert replay(want, spoiled, 1) == ([0, 0, 0, 0, 4, NOT_REACHED], [0, 0, 0, 0, n_public(1, 1) - 1, 0], 4)
    _same_state(c, want)


@pytest.mark.parametrize("signatures", [False, True], ids=["plain", "signatures"])
def test_every_signal_of_batch_0_one_at_a_time(chain, signatures):
    """Signal i of batch 0 plus one (mod r), batches 0 and 1 replayed: what the model says, and in particular the contract's
    root check at signal 1, the signature fields, and `where == i` for everything that is derived."""
    b, _ = _pair(DEPTH, 6)
    root = b.root
    start, publics = chain["start"], chain["publics"]
    sig_fields = {tx_base(BATCH, k) + j for k in range(BATCH) for j in (5, 6, 7)}
    message_fields = {tx_base(BATCH, k) + j for k in range(BATCH) for j in range(5)}
    for i in range(NP):
        spoiled = list(publics[0])
        spoiled[i] = (spoiled[i] + 1) % o.R
        code, at, _ = judge(start, spoiled, BATCH, signatures=signatures, sig_ok=_sig_ok)
        # the model's answers are the ones the contract and the circuit give
        if i == 1:
            assert (code, at) == (2, 1)
        elif i in sig_fields:
            assert (code, at) == ((5, (i - tx_base(BATCH, 0)) // 8) if signatures else (0, 0))
        elif i in message_fields:
            # mostly (4, 0); the first transaction's nonce is overwritten by the second one of the same sender: (4, 2)
            assert (code, at) == (5, (i - tx_base(BATCH, 0)) // 8) if signatures else code == 4 and at in (0, 2)
        else:
            assert (code, at) == (4, i)
        got = b.replay([spoiled, publics[1]], BATCH, signatures=signatures)
        if code == 0:                                                 # a signature nobody looks at: both batches apply; start over
            assert got == ([0, 0], [0, 0], 2), i
            b, _ = _pair(DEPTH, 6)
        else:
            assert got == ([code, NOT_REACHED], [at, 0], 0), i
    assert b.root == root and b.info()["applied"] == 0
    _same_state(b, start)


@pytest.mark.parametrize("form", ["host", "device"])
def test_a_refusal_in_the_middle(chain, form):
    """A recipient path element of batch 3 is wrong: three batches are applied and the ledger is the model after three.  Batch 2
    and batch 4 both write leaves 4 and 5, so "holds the last version of its node" differs between the planned list and the
    stored prefix: stale tables would leave batch 4's nodes in the tree, which shows as a wrong root and wrong paths."""
    publics = chain["publics"]
    touched = lambda p: {p[tx_base(BATCH, k) + j] for k in range(BATCH) for j in (0, 1)}
    assert touched(publics[2]) & touched(publics[4]) == {4, 5}
    at = 1 + (17 + DEPTH) * BATCH + 1 * DEPTH + 1                     # txRecipientPathElements[1][1]
    spoiled = [list(p) for p in publics]
    spoiled[3][at] = (spoiled[3][at] + 1) % o.R
    b, _ = _pair(DEPTH, 6)
    want = ([0, 0, 0, 4, NOT_REACHED, NOT_REACHED], [0, 0, 0, at, 0, 0], 3)
    assert replay(copy.deepcopy(chain["start"]), spoiled, BATCH) == want
    assert _replay(b, form, spoiled, BATCH) == want
    _same_state(b, chain["states"][3])
    assert b.info() == {"depth": 3, "accounts": 6, "applied": 6, "batches": 3}
    assert _replay(b, form, publics[3:], BATCH) == ([0] * 3, [0] * 3, 3)
    _same_state(b, chain["states"][6])
    assert b.root == chain["a"].root


def test_a_refused_proof_and_a_stale_root(chain):
    publics = chain["publics"]
    b, _ = _pair(DEPTH, 6)
    assert b.replay(publics, BATCH, proof_verdicts=[0, 0, 4, 0, 0, 0]) == ([0, 0, 3, NOT_REACHED, NOT_REACHED, NOT_REACHED], [0] * 6, 2)
    _same_state(b, chain["states"][2])
    # the contract compares the root (RollUp.sol:92) before it asks the verifier (:96)
    stale = [list(p) for p in publics[2:]]
    stale[0][1] = (stale[0][1] + 1) % o.R
    assert judge(chain["states"][2], stale[0], BATCH, proof_verdict=4)[:2] == (2, 1)
    assert b.replay(stale, BATCH, proof_verdicts=[4, 0, 0, 0]) == ([2] + [NOT_REACHED] * 3, [1, 0, 0, 0], 0)
    # ... and what cannot be applied at all comes before both
    stale[0][tx_base(BATCH, 1) + 1] = 6
    assert b.replay(stale, BATCH, proof_verdicts=[4, 0, 0, 0]) == ([1] + [NOT_REACHED] * 3, [tx_base(BATCH, 1) + 1, 0, 0, 0], 0)
    _same_state(b, chain["states"][2])
    assert b.replay(publics[2:], BATCH, proof_verdicts=[0] * 4)[2] == 4 and b.root == chain["a"].root


def test_two_runs_with_a_deposit_between_them_equal_one_model_run():
    b, m = _pair(DEPTH, 4)
    q = _Queue(5)
    q.tx(0, 1), q.tx(1, 2), q.tx(2, 3), q.tx(3, 0)
    assert b.replay(publish(m, q.rows, BATCH), BATCH, signatures=True) == ([0, 0], [0, 0], 2)
    _same_state(b, m)
    for row in ((4, keypair(4)[1], 500, 0), (1, keypair(1)[1], 77, m.accounts[1][3])):          # a new account; an overwritten balance
        b.deposit(*row)
        m.deposit(*row)
    q.rows = []
    q.tx(4, 1), q.tx(1, 4), q.tx(0, 4), q.tx(2, 2)
    assert b.replay(publish(m, q.rows, BATCH), BATCH, signatures=True) == ([0, 0], [0, 0], 2)
    _same_state(b, m)
    assert b.info() == {"depth": 3, "accounts": 5, "applied": 8, "batches": 4}


def test_argument_errors_leave_everything_as_it_was(chain):
    import zkr_hip
    L = zkr_hip.lib()
    b, m = _pair(DEPTH, 6)
    buf = le(v for p in chain["publics"][:2] for v in p)
    w, ptrs = _witnesses(chain["publics"][:2])
    verdicts, where, applied = ctypes.create_string_buffer(b"\x07\x07", 2), (ctypes.c_uint32 * 2)(9, 9), ctypes.c_size_t(7)

    def refused(rc, word):
        assert rc == -5 and word in L.zkr_last_error(), L.zkr_last_error()
        assert verdicts.raw == b"\x07\x07" and list(where) == [9, 9] and applied.value == 0
        applied.value = 7
    host = lambda h, p, n, batch, flags, v: L.zkr_ledger_replay(h, p, n, batch, None, flags, v, where, ctypes.byref(applied), None)
    refused(host(b._h, None, 2, BATCH, 0, verdicts), b"null")
    refused(host(None, buf, 2, BATCH, 0, verdicts), b"null")
    refused(host(b._h, buf, 2, BATCH, 0, None), b"null")
    refused(host(b._h, buf, 2, 0, 0, verdicts), b"batch")
    refused(host(b._h, buf, 2, BATCH, 2, verdicts), b"flags")
    refused(host(b._h, buf, (1 << 21) + 1, BATCH, 0, verdicts), b"2^22")
    dev = lambda arr, n: L.zkr_ledger_replay_device(b._h, arr, n, BATCH, None, 0, verdicts, where, ctypes.byref(applied), None)
    refused(dev(None, 2), b"null")
    refused(dev((ctypes.c_void_p * 2)(ptrs[0], None), 2), b"witness 1")
    _same_state(b, m)
    assert b.info()["applied"] == 0
    with pytest.raises(ValueError):
        b.replay(chain["publics"][:2], BATCH, proof_verdicts=[0])
    assert b.replay([], BATCH) == ([], [], 0) and b.replay_device([], BATCH) == ([], [], 0)
    assert b.replay_device(ptrs, BATCH) == ([0, 0], [0, 0], 2)


def test_through_real_proofs():
    """sequence -> witnesses -> prove_batch_device -> verify_each_device on the operator's side; the follower hands the same
    witness pointers and the verifier's verdicts to replay_device, signatures included, and ends in the operator's root."""
    import torch
    import zkr_hip
    from zkr_hip import rollup as n
    c = n.RollupCircuit(2, 3)
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(c.r1cs(), toxic=[2, 3, 5, 7, 11])
    a, model = _pair(3, 5)
    follower, _ = _pair(3, 5)
    q = _Queue(5)
    q.tx(0, 1), q.tx(1, 0), q.tx(2, 2), q.tx(3, 4), q.tx(4, 3), q.tx(0, 4), q.tx(0, 2), q.tx(3, 2)
    status, inputs, _ = a.sequence(q.rows, 2)
    assert status == [0] * 8
    stream = torch.cuda.current_stream().cuda_stream
    wit = c.calculate_witness_batch_from_device(inputs, stream=stream)
    ptrs = [wit[i].data_ptr() for i in range(4)]
    proofs = key.prove_batch_device(ptrs, [5, 6, 7, 8], [9, 10, 11, 12])
    with zkr_hip.VerifyingKey(vk_bin) as vk:
        verdicts = vk.verify_each_device(proofs, ptrs)
    assert verdicts == [0, 0, 0, 0]
    assert follower.replay_device(ptrs, 2, proof_verdicts=verdicts, signatures=True, stream=stream) == ([0] * 4, [0] * 4, 4)
    assert follower.root == a.root
    publish(model, q.rows, 2)
    _same_state(follower, model)
