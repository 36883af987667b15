"""GPU: the ledger's book (include/zkr.h zkr_ledger_book_open .. zkr_ledger_book_blob; csrc/zkr_book.hip) against
tests/book_model.py -- RollUp.sol's deposit, withdraw / withdrawAll and accuredFees one call at a time over oracle/rollup.py.
After every step the whole state is compared with the model as tests/test_gpu_ledger_state.py does (records, root, the stored
tree byte for byte, the audit), and with it index_of, nullifiers_used, fees and book_info.  The salt is passed, so the model
knows where a nullifier's probe starts (book_model.slot_of) and the tests can craft nullifiers that share a slot or wrap."""
import copy

import pytest

import rollup as o
from book_model import NONE, Book, build_blob, slot_of
from replay_model import publish
from sequencer_model import P250, Model, keypair
from test_gpu_ledger_state import _full_state, _queue, _refused, _seq_both, _tree_bytes
from test_gpu_sequencer import _pair

pytestmark = pytest.mark.gpu

SALT = 0x5A4B00B00C5EED01
BAL = 1000


class Pair:
    """A ledger with an open book and the model beside it; `builds` counts what book_info must report."""

    def __init__(self, depth, n_accounts, cap_log2=None, balance=BAL):
        self.a, m = _pair(depth, n_accounts, balance)
        self.b = Book(m, cap_log2=cap_log2 or 10)
        self.a.open_book(nullifier_cap_log2=cap_log2, salt=SALT)
        self.builds = 1

    def check(self, extra_keys=(), extra_nullifiers=()):
        a, b = self.a, self.b
        _full_state(a, b.m)
        keys = [tuple(b.m.accounts[i][:2]) for i in range(len(b.m.accounts))] + list(extra_keys) + [keypair(900)[1], (o.R, 1), (1, o.R + 5)]
        assert a.index_of(keys) == b.index_of(keys)
        nulls = list(b.nullifiers) + list(extra_nullifiers) + [123456789, o.R]
        assert a.nullifiers_used(nulls) == b.nullifiers_used(nulls)
        assert a.fees() == b.fees
        assert a.book_info() == b.info(self.builds)

    def deposit(self, pubs, values):
        got = self.a.deposit_calls(pubs, values)
        assert got == self.b.deposit_calls(pubs, values)
        self.b.settle()
        return got

    def withdraw(self, publics, amounts=None, proofs=None):
        got = self.a.withdraw_calls(publics, amounts, proofs)
        assert got == self.b.withdraw_calls(publics, amounts, proofs)
        self.b.settle()
        return got

    def event_deposit(self, index, pub, balance, nonce=0):
        """Event-form deposit: the key table goes stale when it inserts an account or moves a key, and is built again."""
        stale = index >= len(self.b.m.accounts) or tuple(self.b.m.accounts[index][:2]) != tuple(pub)
        self.a.deposit(index, pub, balance, nonce), self.b.m.deposit(index, pub, balance, nonce)
        self.builds += 1 if stale else 0


def pub(i):
    return keypair(i)[1]


# ------------------------------------------------------------------------------------------------ key table
@pytest.mark.parametrize("depth,n", [(1, 2), (3, 8), (6, 40)])
def test_key_table_finds_every_account_and_nothing_else(depth, n):
    """2 accounts in 4 slots; 8 in 16, where chains and the wrap at the table's end are certain; 40 in 128."""
    p = Pair(depth, n)
    p.check()
    assert p.a.index_of([pub(i) for i in range(n)]) == list(range(n))
    assert p.a.index_of([pub(n), (pub(0)[0], pub(1)[1]), (pub(0)[0] + o.R, pub(0)[1])]) == [None, None, None]
    assert p.a.index_of([]) == [] and p.a.nullifiers_used([]) == []
    status, events = p.deposit([pub(n - 1), pub(0), pub(n - 1)], [5, 6, 7])      # calls by key land on the accounts the events made
    assert status == [0, 0, 0] and events[2] == (n - 1,) + tuple(pub(n - 1)) + (BAL + 12, 0)
    p.check()


def test_two_accounts_with_one_key_and_a_key_that_changes():
    p = Pair(3, 4)
    p.event_deposit(4, pub(1), 77)                                    # the contract cannot do this, the event form can
    p.check()
    assert p.a.index_of([pub(1)]) == [1] and p.builds == 2           # the lowest index owns the key
    status, events = p.deposit([pub(1)], [1])
    assert status == [0] and events[0][0] == 1
    p.event_deposit(1, pub(50), BAL + 1)                              # account 1 moves to another key: 4 is what is left under the old one
    p.check(extra_keys=[pub(50)])
    assert p.a.index_of([pub(1), pub(50)]) == [4, 1] and p.builds == 3
    p.event_deposit(4, pub(51), 77)                                   # and now nobody holds it
    assert p.a.index_of([pub(1), pub(51)]) == [None, 4]
    p.event_deposit(0, pub(0), 5, 9)                                  # balance and nonce only: nothing goes stale
    p.check()
    assert p.builds == 4
    verdicts, _ = p.withdraw([pub(1) + (1,), pub(51) + (2,)], [1, 1])
    assert verdicts == [4, 0]
    p.check()


# ------------------------------------------------------------------------------------------------ nullifier set
def _crafted(mask, slot, count, start):
    """`count` nullifiers from `start` on whose probes begin at `slot` of a table of mask + 1 slots."""
    out, v = [], start
    while len(out) < count:
        if slot_of(v, SALT, mask) == slot:
            out.append(v)
        v += 1
    return out


def test_nullifier_set_grows_and_keeps_every_nullifier():
    """Four slots to begin with: the table doubles at the 3rd, 5th, 9th and 17th nullifier.  Nullifiers that differ only in word 0
    and only in word 7, 0 and r - 1, and nullifiers whose probes all start at the last slot of the table they are inserted into."""
    p = Pair(3, 2, cap_log2=2, balance=10 ** 6)
    assert p.a.book_info()["nullifier_capacity"] == 4
    base = 0x0123456789ABCDEF << 64
    wrap4, wrap8, wrap64 = _crafted(3, 3, 2, 1000), _crafted(7, 7, 2, 2000), _crafted(63, 63, 4, 3000)
    singles = wrap4 + wrap8 + [0, o.R - 1, base, base + 1, base + (1 << 224), base + 2, base + (2 << 224), 5, 6, 7, 8, 9] + wrap64
    assert len(singles) == 20 and len(set(singles)) == 20
    caps = []
    for k, v in enumerate(singles):
        verdicts, _ = p.withdraw([pub(k % 2) + (v,)], [1])
        assert verdicts == [0]
        caps.append(p.a.book_info()["nullifier_capacity"])
        assert p.a.nullifiers_used(singles) == [True] * (k + 1) + [False] * (len(singles) - k - 1)
        if k in (1, 2, 4, 8, 16, 19):
            p.check(extra_nullifiers=singles)
    assert caps == [4, 4, 8, 8] + [16] * 4 + [32] * 8 + [64] * 4
    verdicts, _ = p.withdraw([pub(0) + (o.R,), pub(0) + (o.R + 5,), pub(0) + (5,)], [1, 1, 1])
    assert verdicts == [1, 1, 2]                                      # r + 5 is no spent 5: it is no signal at all
    # one list that makes the table double twice while it is inserted
    more = _crafted(255, 255, 6, 9000) + list(range(100, 140))
    verdicts, _ = p.withdraw([pub(k % 2) + (v,) for k, v in enumerate(more)], [1] * len(more))
    assert verdicts == [0] * len(more) and p.a.book_info()["nullifier_capacity"] == 256
    p.check(extra_nullifiers=more)


# ------------------------------------------------------------------------------------------------ order within a list
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_lists_of_every_length_against_the_model(n):
    """One wavefront, its neighbour, a block of 256 and its neighbour; copies at positions 63 / 64 and 255 / 256 where they exist."""
    p = Pair(4, 5, balance=10 ** 6)
    nulls = [10 ** 9 + i for i in range(n)]
    for at in (64, 256):
        if at < n:
            nulls[at] = nulls[at - 1]
    verdicts, events = p.withdraw([pub(i % 7) + (nulls[i],) for i in range(n)], [1 + i % 3 for i in range(n)])   # keys 5 and 6 are not registered
    assert len(verdicts) == n and all(v == (2 if i in (64, 256) and nulls[i - 1] == nulls[i] and (i - 1) % 7 < 5 else 4 if i % 7 >= 5 else 0) for i, v in enumerate(verdicts))
    p.check()
    keys = [pub(i % 9) for i in range(n)]                             # four keys that are new, each many times
    status, events = p.deposit(keys, [2 + i % 5 for i in range(n)])
    assert status == [0] * n
    assert [e[0] for e in events] == [i % 9 for i in range(n)]
    p.check()


def test_one_nullifier_seventy_times_is_spent_once():
    p = Pair(3, 3)
    verdicts, events = p.withdraw([pub(i % 3) + (4242,) for i in range(70)], [1] * 70)
    assert verdicts == [0] + [2] * 69 and events[0][0] == 0
    p.check()
    verdicts, _ = p.withdraw([pub(i % 3) + (4242,) for i in range(70)])       # and never again
    assert verdicts == [2] * 70
    # the first 66 copies are refused, each for another reason: the first one that passes every check spends it
    publics = [(o.R, 1, 77)] + [pub(7) + (77,)] + [pub(0) + (77,)] * 68
    amounts = [1, 1] + [BAL] * 64 + [1] * 4
    verdicts, _ = p.withdraw(publics, amounts, [0, 0] + [1] * 64 + [0] * 4)
    assert verdicts == [1, 4] + [3] * 64 + [0] + [2] * 3
    p.check()


def test_refused_leader_repeated_withdrawals_and_withdraw_all():
    p = Pair(3, 4)
    publics = [pub(1) + (77,), pub(2) + (77,), pub(3) + (77,), pub(1) + (78,), pub(0) + (78,)]
    verdicts, events = p.withdraw(publics, [BAL + 1, 20, 1, 5, 5])       # the leader is refused for its balance and spends nothing
    assert verdicts == [5, 0, 2, 0, 2] and events[1] == (2,) + tuple(pub(2)) + (BAL - 20, 0)
    p.check()
    verdicts, events = p.withdraw([pub(0) + (100 + i,) for i in range(6)], [300] * 6)     # until the balance runs out
    assert verdicts == [0, 0, 0, 5, 5, 5] and events[2][3] == BAL - 900
    assert p.a.nullifiers_used([100, 101, 102, 103]) == [True, True, True, False]
    p.check()
    verdicts, events = p.withdraw([pub(3) + (200,), pub(3) + (201,), pub(0) + (202,)])    # withdrawAll
    assert verdicts == [0, 6, 0] and events[0][3] == 0 and events[2][3] == 0
    p.check()


def test_a_key_that_is_new_twice_in_one_list_and_a_tree_that_fills():
    p = Pair(2, 2)
    status, events = p.deposit([pub(5), pub(5), pub(0), pub(6), pub(7), pub(6), pub(5)], [P250, 4, 1, 2, 3, P250 - 2, 6])
    assert status == [1, 0, 0, 0, 2, 3, 0]
    assert events[1] == (2,) + tuple(pub(5)) + (4, 0) and events[6] == (2,) + tuple(pub(5)) + (10, 0) and events[3][0] == 3
    p.check(extra_keys=[pub(7)])
    assert p.a.index_of([pub(5), pub(6), pub(7)]) == [2, 3, None] and p.builds == 1      # the new accounts were inserted, nothing was rebuilt


# ------------------------------------------------------------------------------------------------ determinism
def test_the_same_lists_on_two_fresh_ledgers():
    outs = []
    for _ in range(2):
        p = Pair(4, 6)
        keys = [pub(i % 11) for i in range(130)]
        got = [p.deposit(keys, [1 + i for i in range(130)])]
        nulls = [500 + (i * 7) % 90 for i in range(200)]
        got.append(p.withdraw([pub(i % 12) + (nulls[i],) for i in range(200)], [3] * 200))
        p.check()
        outs.append((got, _tree_bytes(p.a), p.a.book_blob(), p.a.snapshot()))
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------ blob
def test_blob_round_trip_beside_a_snapshot():
    from zkr_hip import rollup as nat
    p = Pair(3, 4, cap_log2=2)
    p.withdraw([pub(i % 4) + (o.R - 1 - i,) for i in range(7)], [1] * 7)
    p.b.fees += _sequence(p, [(0, 1), (1, 2)])
    blob, snap = p.a.book_blob(), p.a.snapshot()
    assert blob == p.b.blob() and nat.Ledger.book_blob_check(blob) == ({"nullifiers": 7, "fees": p.b.fees}, None)
    q = copy.copy(p)
    q.a, q.builds = nat.Ledger.restore(snap), 1
    _refused(-5, lambda: q.a.fees(), "no open book")
    _refused(-5, lambda: q.a.withdraw_calls([pub(0) + (1,)], [1]), "no open book")
    _refused(-5, lambda: q.a.open_book(blob[:-1], salt=SALT), "length")
    twice = build_blob(p.b.nullifiers[:3] + p.b.nullifiers[1:2] + p.b.nullifiers[3:], p.b.fees)
    assert nat.Ledger.book_blob_check(twice)[1] is None                # well formed: the repeat shows only in the set's own table
    _refused(-2, lambda: q.a.open_book(twice, salt=SALT), "repeats")
    _refused(-5, lambda: q.a.book_info(), "no open book")               # a refused open leaves no book behind
    q.a.open_book(blob, nullifier_cap_log2=2, salt=SALT + 2)
    _refused(-5, lambda: q.a.open_book(blob), "open already")
    q.check()
    assert q.a.book_blob() == blob and q.a.snapshot() == snap
    same = [pub(1) + (o.R - 3,), pub(1) + (99,), pub(9) + (98,)]      # the two resume to the same answers
    assert p.withdraw(same, [1, 1, 1]) == q.a.withdraw_calls(same, [1, 1, 1])
    assert p.deposit([pub(8), pub(0)], [5, 5]) == q.a.deposit_calls([pub(8), pub(0)], [5, 5])
    p.check(), q.check()
    assert q.a.book_blob() == p.a.book_blob()


# ------------------------------------------------------------------------------------------------ checkpoints, fees
def _sequence(p, pairs):
    """One sequence call on the ledger and the model: -> the fees of what was applied."""
    rows = _queue(p.b.m, pairs)
    status, _, consumed = _seq_both(p.a, p.b.m, rows)
    assert status == [0] * len(rows) and consumed == len(rows)
    return sum(r[3] for r in rows)


def test_rollback_puts_the_book_back_and_release_keeps_it():
    p = Pair(3, 4, cap_log2=2)
    p.withdraw([pub(0) + (1,), pub(1) + (2,)], [1, 1])
    p.b.fees += _sequence(p, [(0, 1), (1, 0)])
    p.check()
    at = copy.deepcopy(p.b)
    _refused(-5, lambda: p.a.fees(reset=True) if p.a.checkpoint() else None, "checkpoint")
    cp = p.a.journal_info()[0]
    assert cp == 1
    cp = p.a.checkpoint()                                               # nested: rolled back to below, the outer one released
    p.deposit([pub(7), pub(0), pub(7)], [10, 10, 10])
    p.withdraw([pub(7) + (3,), pub(2) + (4,), pub(3) + (5,), pub(3) + (6,)], [5, 5, 5, 5])
    p.b.fees += _sequence(p, [(2, 3), (3, 0)])
    p.check()
    assert p.a.book_info()["nullifier_capacity"] == 16 and p.a.index_of([pub(7)]) == [4]
    p.a.rollback(cp)
    p.b, p.builds = copy.deepcopy(at), p.builds + 1
    p.b.cap = 16                                                        # a table that has grown stays grown
    p.check(extra_keys=[pub(7)], extra_nullifiers=[3, 4, 5, 6])
    assert p.a.index_of([pub(7)]) == [None] and p.a.nullifiers_used([1, 2, 3, 6]) == [True, True, False, False]
    verdicts, _ = p.withdraw([pub(2) + (4,), pub(2) + (1,)], [5, 5])   # a rolled-back nullifier is free again
    assert verdicts == [0, 2]
    status, events = p.deposit([pub(8), pub(7)], [1, 2])               # and a rolled-back key is new again, behind another one
    assert status == [0, 0] and [e[0] for e in events] == [4, 5]
    p.check()
    p.a.release(cp)
    for open_cp in range(1, cp):
        p.a.release(open_cp)
    assert p.a.journal_info() == (0, 0)
    p.check()
    assert p.a.fees(reset=True) == p.b.fees and p.a.fees() == 0
    p.b.fees = 0
    p.check()


def test_fees_follow_sequence_and_replay():
    p = Pair(3, 5)
    p.b.fees += _sequence(p, [(0, 1), (1, 2), (2, 3), (3, 4)])
    p.check()
    rows = [[0, 1, 5, 2, 77, 0, 0, 0], [1, 0, 0, 0, 3, 0, 0, 0], [4, 4, 1, 9, 1, 0, 0, 0], [2, 3, 7, 1, 8, 0, 0, 0]]
    publics = publish(p.b.m, rows, 2)                                   # the contract applies whatever was proved
    assert p.a.replay(publics + publics[:1], 2) == ([0, 0, 2], [0, 0, 1], 2)    # a batch from a root long gone: its fees are not accrued
    p.b.fees += 2 + 0 + 9 + 1
    p.check()
    import torch
    more = publish(p.b.m, [[3, 0, 1, 4, 9, 0, 0, 0], [0, 3, 1, 6, 78, 0, 0, 0]], 2)
    wit = torch.frombuffer(bytearray(bytes(32) + b"".join(int(v).to_bytes(32, "little") for v in more[0])), dtype=torch.uint8).cuda()
    assert p.a.replay_device([wit.data_ptr()], 2) == ([0], [0], 1)
    p.b.fees += 10
    p.check()
    assert p.a.fees(reset=True) == p.b.fees and p.a.fees() == 0


# ------------------------------------------------------------------------------------------------ signals in device memory
def test_withdraw_calls_from_witnesses_in_device_memory():
    """86 witnesses: 258 signal words, the smallest list that spans two blocks of the gather kernel."""
    from zkr_hip import rollup as nat
    n = 86
    c = nat.WithdrawCircuit()
    cases = [{"privateKey": nat.format_priv_key(keypair(i % 5)[0]), "nullifier": 7000 + (i if i % 10 else 0)} for i in range(n)]   # key 4 is not registered
    wit = c.calculate_witness_batch_device(cases)
    publics = [tuple(pub(i % 5)) + (cases[i]["nullifier"],) for i in range(n)]
    assert [tuple(c.public_signals(bytes(r))) for r in wit[:3].cpu().numpy()] == publics[:3]
    amounts, proofs = [1 + i % 4 for i in range(n)], [1 if i % 13 == 5 else 0 for i in range(n)]
    p, q = Pair(3, 4), Pair(3, 4)
    got = p.a.withdraw_calls_device([wit[i].data_ptr() for i in range(n)], amounts, proofs)
    assert got == q.withdraw(publics, amounts, proofs)
    assert sorted(set(got[0])) == [0, 2, 3, 4]
    p.b = q.b
    p.check()
    assert p.a.book_blob() == q.a.book_blob()
    _refused(-5, lambda: p.a.withdraw_calls_device([wit[0].data_ptr(), 0]), "null pointer")
