"""CPU: the host pass of the transaction sequencer (include/zkr.h zkr_sequence_plan_host; csrc/sequencer_plan.cpp) against the
rule list applied one transaction at a time in Python (tests/sequencer_model.py over oracle/rollup.py): the status of every
rule, what a rejection does to the transactions behind it, whole batches only, and the three look-up tables against an
exhaustive search.  Rule 10 comes in as a verdict byte here (the signature kernel is tests/test_gpu_sequencer.py's matter): the
S field of a row is 1 where the verdict is "holds"."""
import copy

import pytest

import rollup as o
from sequencer_model import NOT_REACHED, P250, Model, apply_tx, brute_tables, keypair, signed_row, status_of

BAL = 10_000


def _model(depth, n_accounts, with_tree=False, rich=None):
    m = Model(depth, with_tree=with_tree)
    for i in range(n_accounts):
        m.deposit(i, (11 + i, 22 + i), P250 - 5 if i == rich else BAL)
    return m


def _row(frm, to, amount, fee, nonce, ok=1):
    return [frm, to, amount, fee, nonce, 0, 0, ok]


def _verdict(row, pub):
    return row[7] != 0


def _plan(m, rows, batch):
    from zkr_hip import rollup as n
    return n.sequence_plan_host(m.depth, m.records(), rows, [r[7] != 0 for r in rows], batch)


BREAKS = [
    (1, _row(9, 1, 5, 1, 1)),                          # no such sender
    (1, _row(o.R + 2, 1, 5, 1, 1)),                    # ... an index that only reads as account 2 modulo r
    (2, _row(2, 4, 5, 1, 1)),                          # no such recipient (4 accounts: 0..3)
    (3, _row(2, 1, o.R, 1, 1)),                        # amount is no field element
    (3, _row(2, 1, P250, 1, 1)),                       # amount below r but past the circuit's 250 bits
    (3, _row(2, 1, 5, P250, 1)),
    (3, _row(2, 1, 5, 1, P250 + 1)),
    (3, [2, 1, 5, 1, 1, 0, o.R, 1]),                   # R8y is no field element
    (4, _row(2, 1, 0, 1, 1)),
    (5, _row(2, 1, 5, 0, 1)),
    (6, _row(2, 1, BAL - 1, 1, 1)),                    # balance == amount + fee: the circuit wants it strictly greater
    (6, _row(2, 1, BAL, 1, 1)),
    (7, _row(2, 1, 5000, 14, 1)),                      # (5000 div 1000) * 3 = 15
    (8, _row(2, 1, 5, 1, 2)),
    (8, _row(2, 1, 5, 1, 0)),
    (9, _row(2, 3, 10, 1, 1)),                         # account 3 holds 2^250 - 5
]


@pytest.mark.parametrize("code,bad", BREAKS, ids=["rule%d_%d" % (c, i) for i, (c, _) in enumerate(BREAKS)])
def test_a_transaction_that_breaks_one_rule_gets_that_rules_code_and_its_neighbours_are_unaffected(code, bad):
    m = _model(3, 4, rich=3)
    rows = [_row(0, 1, 7, 1, 1), bad, _row(1, 2, 3, 1, 1), _row(2, 0, 4, 1, 1)]   # the last one: account 2's nonce was not consumed
    assert status_of(m.accounts, bad, _verdict) == code
    got, consumed, _ = _plan(m, rows, 1)
    assert got == [0, code, 0, 0] and consumed == 4
    want, _, want_consumed, _ = m.sequence(rows, 1, _verdict)
    assert (got, consumed) == (want, want_consumed)


def test_rule_7_boundary_and_rule_6_just_above():
    m = _model(2, 3)
    rows = [_row(0, 1, 5000, 15, 1), _row(1, 2, 999, 1, 1), _row(2, 0, BAL + 999 - 40, 39, 1)]  # fee exactly the minimum; none below 1000; balance = amount + fee + 1
    got, consumed, _ = _plan(m, rows, 1)
    assert got == [0, 0, 0] == m.sequence(rows, 1, _verdict)[0] and consumed == 3


def test_a_rejection_changes_what_follows():
    """A sender's second transaction is valid only because the first was rejected: its nonce was not consumed."""
    m = _model(2, 3)
    rows = [_row(0, 1, 5, 1, 1, ok=0), _row(0, 1, 5, 1, 1), _row(0, 2, 5, 1, 2), _row(0, 2, 5, 1, 2), _row(1, 2, 5, 1, 1)]
    got, consumed, _ = _plan(m, rows, 1)
    assert got == [10, 0, 0, 8, 0] and consumed == 5
    assert got == m.sequence(rows, 1, _verdict)[0]
    # the balance a rejected transaction did not spend is still there for the next one
    m2 = _model(2, 2)
    rows = [_row(0, 1, BAL - 32, 30, 7), _row(0, 1, BAL - 32, 30, 1), _row(0, 1, 1, 1, 2), _row(1, 0, 1, 1, 1)]
    assert _plan(m2, rows, 1)[0] == [8, 0, 6, 0]


def test_only_whole_batches_are_applied_and_the_rest_is_not_reached():
    """A = 5 accepted at batch 2: four are applied, `consumed` stands behind the fourth, everything from there on is 255 -- the
    fifth accepted transaction and the rejected one before it included."""
    m = _model(3, 5)
    rows = [_row(0, 1, 5, 1, 1), _row(1, 2, 5, 1, 1), _row(2, 3, 5, 1, 9), _row(2, 3, 5, 1, 1), _row(3, 4, 5, 1, 1), _row(4, 0, 0, 1, 1), _row(4, 0, 5, 1, 1)]
    got, consumed, tables = _plan(m, rows, 2)
    assert got == [0, 0, 8, 0, 0, NOT_REACHED, NOT_REACHED] and consumed == 5
    assert len(tables[0][0]) == 8                                       # 2 x 4 updates
    want, _, want_consumed, idx = m.sequence(rows, 2, _verdict)
    assert (got, consumed) == (want, want_consumed) and idx == [0, 1, 1, 2, 2, 3, 3, 4]
    assert m.accounts[4][2] == BAL + 5 and m.accounts[4][3] == 0       # the fifth was not applied
    # batch 3: one whole batch; batch 6: none, nothing decided
    assert _plan(_model(3, 5), rows, 3)[:2] == ([0, 0, 8, 0] + [NOT_REACHED] * 3, 4)
    got6, consumed6, tables6 = _plan(_model(3, 5), rows, 6)
    assert got6 == [NOT_REACHED] * 7 and consumed6 == 0 and tables6[0][0] == []


def _mixed_queue(depth):
    """The interactions the level-by-level schedule has to get right, over min(2^depth, 6) accounts: the same sender twice in a
    row, sibling leaves (2j, 2j+1) in consecutive transactions, from == to, a recipient that is the previous sender, and (depth
    3: leaves 6 and 7) a subtree no transaction touches."""
    n = min(1 << depth, 6)
    nonce = [0] * n
    rows = []

    def tx(frm, to):
        frm, to = frm % n, to % n
        nonce[frm] += 1
        rows.append(_row(frm, to, 3, 1, nonce[frm]))
    tx(0, 1), tx(0, 1)              # the same sender twice in a row; siblings 0 and 1
    tx(1, 0)                        # the recipient is the previous sender
    tx(2, 3), tx(3, 2)              # sibling leaves in consecutive transactions, both ways
    tx(1, 1)                        # from == to
    tx(4, 5), tx(5, 5), tx(0, 4), tx(3, 0), tx(2, 2), tx(2, 1)
    return n, rows


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_look_up_tables_against_an_exhaustive_search(depth):
    n, rows = _mixed_queue(depth)
    m = _model(depth, n)
    got, consumed, tables = _plan(m, rows, 1)
    assert got == [0] * len(rows) and consumed == len(rows)
    idx = [v for r in rows for v in r[:2]]
    want = brute_tables(depth, idx)
    assert tables == want
    flat0 = [p for lv in tables[0] for p in lv]
    assert -1 in flat0 and any(p >= 0 for p in flat0)                   # both sources of a sibling occur: the stored tree, an earlier update
    if depth == 3:                                                      # nothing ever names the untouched subtree: its sibling reads the stored node
        assert all(tables[0][1][u] == -1 for u in range(len(idx)) if idx[u] >> 1 == 2)


def test_refused_arguments():
    from zkr_hip import ZkrError
    from zkr_hip import rollup as n
    rec = [[1, 2, BAL, 0], [3, 4, BAL, 0]]
    for depth, records, batch in ((0, rec, 1), (25, rec, 1), (1, rec + rec, 1), (2, rec, 0), (2, [[1, 2, o.R, 0], [3, 4, BAL, 0]], 1), (2, [[1, 2, BAL, P250], [3, 4, BAL, 0]], 1)):
        with pytest.raises(ZkrError) as e:
            n.sequence_plan_host(depth, records, [_row(0, 1, 5, 1, 1)], [1], batch)
        assert e.value.code == -5


def test_stale_path_is_refused_by_the_host_witness_builder():
    """Negative control of the end-to-end GPU check: inputs whose sender path was read from the tree BEFORE the previous
    transaction's updates do not satisfy the circuit (zkr_rollup_witness refuses them), while the model's do."""
    from zkr_hip import ZkrError
    from zkr_hip import rollup as n
    depth = 3
    m = Model(depth)
    for i in range(3):
        m.deposit(i, keypair(i)[1], 1000)
    rows = [signed_row(0, 1, 10, 1, 1), signed_row(1, 0, 20, 2, 1)]      # the second sender is the first one's sibling leaf and recipient
    stale_tree = copy.deepcopy(m.tree)
    fresh = copy.deepcopy(m)
    txs = [apply_tx(m.tree, m.accounts, r) for r in rows]
    c = n.RollupCircuit(2, depth)
    good = c.flatten_inputs({f: [t[f] for t in txs] for f in n.TX_INPUT_FIELDS})
    status, inputs, consumed, _ = fresh.sequence(rows, 2)
    assert status == [0, 0] and consumed == 2 and inputs == [good] == [o.batch_public_signals(txs)[1:]]
    w = c.calculate_witness(good)
    assert c.public_signals(w)[0] == m.tree.root
    assert stale_tree.path(1) != txs[1]["txSenderPathElements"]
    txs[1]["txSenderPathElements"] = stale_tree.path(1)
    with pytest.raises(ZkrError) as e:
        c.calculate_witness(c.flatten_inputs({f: [t[f] for t in txs] for f in n.TX_INPUT_FIELDS}))
    assert e.value.code == -7 and "sender leaf" in str(e.value)


def test_the_models_transition_is_the_oracles_own():
    """tests/sequencer_model.py applies a signed transaction as oracle/rollup.py process_tx_inputs does, which signs for itself:
    the same queue through both gives the same circuit inputs (from == to and a rejected transaction included)."""
    m = Model(2)
    for i in range(3):
        m.deposit(i, keypair(i)[1], 1000)
    ref = copy.deepcopy(m)
    rows = [signed_row(0, 1, 10, 1, 1), signed_row(1, 1, 5, 2, 1), signed_row(2, 0, 10, 1, 1, signer=1), signed_row(2, 0, 7, 1, 1)]
    status, inputs, consumed, _ = m.sequence(rows, 1)
    assert status == [0, 0, 10, 0] and consumed == 4
    txs = [o.process_tx_inputs(ref.tree, ref.accounts, r[0], r[1], r[2], r[3], keypair(r[0])[0]) for r, s in zip(rows, status) if s == 0]
    assert inputs == [o.batch_public_signals([t])[1:] for t in txs] and m.tree.root == ref.tree.root == txs[-1]["newBalanceTreeRoot"]
