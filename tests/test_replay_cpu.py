"""CPU: the host pass of a replay (include/zkr.h zkr_replay_plan_host; csrc/sequencer_plan.cpp replay_plan) against the model of
tests/replay_model.py: the contract's arithmetic for published batches (from == to and a sender that is the previous recipient
included), every way into verdict 1 with the signal it names, what the pass does NOT refuse (the operator's rules 4-8), that
planning stops at the first batch that cannot be applied, and the look-up tables against an exhaustive search."""
import copy

import pytest

import rollup as o
from replay_model import cannot_apply, judge, n_public, publish, replay, tx_base
from sequencer_model import NOT_REACHED, P250, Model, brute_tables

BAL = 10_000
DEPTH, BATCH = 3, 2
NP = n_public(BATCH, DEPTH)


def _model(depth, balances):
    m = Model(depth)
    for i, bal in enumerate(balances):
        m.deposit(i, (11 + i, 22 + i), bal, 3 * i)
    return m


def _row(frm, to, amount, fee, nonce):
    return [frm, to, amount, fee, nonce, 5, 6, 7]                    # the pass never looks at R8x R8y S beyond "below r"


def _plan(m, publics, batch):
    from zkr_hip import rollup as n
    return n.replay_plan_host(m.depth, m.records(), publics, batch)


def test_the_pass_does_the_contracts_arithmetic():
    """Six accounts, six batches of two: the same sender twice in a row, from == to, a sender that is the previous recipient,
    sibling leaves; amounts and fees of zero and nonces that do not count up, which the contract applies all the same."""
    start = _model(DEPTH, [BAL] * 6)
    rows = [_row(0, 1, 7, 1, 1), _row(0, 2, 3, 1, 2), _row(2, 3, 5, 2, 9), _row(3, 2, 1, 1, 4), _row(4, 4, 6, 1, 1), _row(5, 4, 0, 0, 0),
            _row(4, 5, BAL - 100, 4, 77), _row(1, 0, 2, 0, 1), _row(2, 2, 0, 3, 1), _row(0, 5, 1, 1, 1), _row(5, 0, 8, 1, 2), _row(3, 1, 9, 9, 9)]
    m = copy.deepcopy(start)
    publics = publish(m, rows, BATCH)
    assert len(publics) == 6 and all(len(p) == NP for p in publics)
    got = _plan(start, publics, BATCH)
    assert got["verdicts"] == [0] * 6 and got["where"] == [0] * 6 and got["planned"] == 6
    assert got["idx"] == [v for r in rows for v in r[:2]]
    acc, want_old, want_new = copy.deepcopy(start.accounts), [], []
    for frm, to, amount, fee, nonce in (r[:5] for r in rows):
        want_old += [list(acc[frm]), list(acc[to])]
        acc[frm][2] -= amount + fee
        acc[frm][3] = nonce
        want_new.append(list(acc[frm]))
        acc[to][2] += amount
        want_new.append(list(acc[to]))
    assert acc == m.accounts                                         # the stepping above is the oracle's own transition
    assert got["old"] == want_old and got["new"] == want_new
    # the old records are what the oracle published as the transactions' inputs
    for k, (s, r) in enumerate(zip(want_old[0::2], want_old[1::2])):
        p, j = publics[k // BATCH], k % BATCH
        assert s[:2] == p[1 + 9 * BATCH + 2 * j:][:2] and s[2] == p[1 + 11 * BATCH + j] and s[3] == p[1 + 12 * BATCH + j]
        assert r[2] == p[1 + (15 + DEPTH) * BATCH + j] and r[3] == p[1 + (16 + DEPTH) * BATCH + j]
    assert got["tables"] == brute_tables(DEPTH, got["idx"])
    assert replay(copy.deepcopy(start), publics, BATCH) == ([0] * 6, [0] * 6, 6)


@pytest.mark.parametrize("depth,batch", [(1, 1), (2, 3)])
def test_tables_at_other_geometries(depth, batch):
    n = 1 << depth
    start = _model(depth, [BAL] * n)
    rows = [_row(t % n, (3 * t + 1) % n, 2, 1, t) for t in range(6)]
    publics = publish(copy.deepcopy(start), rows, batch)
    got = _plan(start, publics, batch)
    assert got["planned"] == 6 // batch and got["tables"] == brute_tables(depth, [v for r in rows for v in r[:2]])


# two batches; the second one is spoiled one signal at a time.  Account 3 holds 2^250 - 5.
GOOD = [_row(0, 1, 7, 1, 1), _row(1, 2, 3, 1, 1), _row(2, 3, 4, 1, 1), _row(0, 0, 5, 1, 2)]
T0, T1 = tx_base(BATCH, 0), tx_base(BATCH, 1)
FIELD_STARTS = [0, 1, 1 + 9 * BATCH, 1 + 11 * BATCH, 1 + 12 * BATCH, 1 + 13 * BATCH, 1 + (13 + DEPTH) * BATCH, 1 + (15 + DEPTH) * BATCH,
                1 + (16 + DEPTH) * BATCH, 1 + (17 + DEPTH) * BATCH, 1 + (17 + 2 * DEPTH) * BATCH, 1 + (18 + 2 * DEPTH) * BATCH]
SPOILED = (
    [("r_at_%d" % i, {i: o.R}, i) for i in FIELD_STARTS] +                                        # every class of signal but txData ...
    [("r_in_txdata_%d" % j, {T1 + j: o.R}, T1 + j) for j in range(8)] +                          # ... and every element of a txData row
    [("r_last_signal", {NP - 1: o.R + 5}, NP - 1), ("r_twice", {NP - 1: o.R, 4: o.R}, 4),
     ("from_is_the_account_count", {T0: 4}, T0), ("to_is_the_account_count", {T1 + 1: 4}, T1 + 1),
     ("from_reads_as_an_account_mod_2_64", {T1: 1 << 64}, T1),
     ("amount_2_250", {T0 + 2: P250}, T0 + 2), ("fee_2_250", {T1 + 3: P250}, T1 + 3), ("nonce_2_250", {T0 + 4: P250}, T0 + 4),
     ("balance_is_amount_plus_fee_less_1", {T0 + 2: BAL + 3}, T0 + 2),                            # account 2 holds BAL + 3 after batch 0; fee 1
     ("balance_short_in_the_second_tx", {T1 + 2: BAL - 8}, T1 + 2),                               # account 0 holds BAL - 8; fee 1
     ("recipient_reaches_2_250", {T0 + 2: 5}, T0 + 2),
     ("range_before_account", {T0 + 2: P250, T1: 9}, T0 + 2), ("first_tx_first", {T0 + 1: 8, T1: 9}, T0 + 1)])


@pytest.mark.parametrize("name,change,where", SPOILED, ids=[s[0] for s in SPOILED])
def test_every_way_into_verdict_1_names_its_signal(name, change, where):
    start = _model(DEPTH, [BAL, BAL, BAL, P250 - 5])
    m = copy.deepcopy(start)
    publics = publish(m, GOOD, BATCH)
    for i, v in change.items():
        publics[1][i] = v
    got = _plan(start, publics, BATCH)
    assert got["verdicts"] == [0, 1] and got["where"] == [0, where] and got["planned"] == 1
    assert got["idx"] == [0, 1, 1, 2] and len(got["new"]) == 4
    want = copy.deepcopy(start)
    assert replay(want, publics, BATCH) == ([0, 1], [0, where], 1)


def test_what_the_contract_applies_the_pass_applies():
    """balance == amount + fee (the sequencer's rule 6 is strict), a recipient that ends at 2^250 - 1, amount 0, fee 0, a nonce
    that goes backwards."""
    start = _model(DEPTH, [BAL, BAL, BAL, P250 - 5])
    rows = [_row(0, 1, BAL - 1, 1, 1), _row(2, 3, 4, 0, 0), _row(0, 2, 0, 0, 0), _row(1, 1, 2 * BAL - 1, 0, 5)]
    m = copy.deepcopy(start)
    publics = publish(m, rows, BATCH)
    assert m.accounts[0][2] == 0 and m.accounts[3][2] == P250 - 1
    got = _plan(start, publics, BATCH)
    assert got["verdicts"] == [0, 0] and got["planned"] == 2
    assert got["new"][0] == [11, 22, 0, 1] and got["new"][3] == [14, 25, P250 - 1, 9] and got["new"][7] == m.accounts[1]
    assert cannot_apply(copy.deepcopy(start.accounts), publics[0], BATCH) is None
    assert replay(copy.deepcopy(start), publics, BATCH) == ([0, 0], [0, 0], 2)


def test_planning_stops_at_the_first_batch_that_cannot_be_applied():
    start = _model(DEPTH, [BAL] * 5)
    rows = [_row(t % 5, (t + 1) % 5, 3, 1, t) for t in range(8)]
    publics = publish(copy.deepcopy(start), rows, BATCH)
    publics[1][T1 + 2] = BAL + 10                                     # more than the sender holds
    publics[3][0] = o.R                                               # never looked at
    got = _plan(start, publics, BATCH)
    assert got["verdicts"] == [0, 1, NOT_REACHED, NOT_REACHED] and got["where"] == [0, T1 + 2, 0, 0] and got["planned"] == 1
    assert got["idx"] == [0, 1, 1, 2] and len(got["old"]) == 4 and len(got["tables"][0][0]) == 4
    assert replay(copy.deepcopy(start), publics, BATCH)[0] == [0, 1, NOT_REACHED, NOT_REACHED]
    # the first transaction of a refused batch is not applied either: the same batch without its second transaction's fault
    first = _plan(start, [publics[1]], BATCH)
    assert first["verdicts"] == [1] and first["idx"] == [] and first["tables"][0][0] == []


def test_the_models_verdicts_beyond_1():
    """replay_model by itself: precedence 1, 2, 3, 5, 4 over one honest batch (no library code involved)."""
    start = _model(DEPTH, [BAL] * 4)
    publics = publish(copy.deepcopy(start), GOOD[:2], BATCH)
    p = publics[0]
    assert judge(start, p, BATCH)[:2] == (0, 0)
    assert judge(start, p, BATCH, proof_verdict=4)[:2] == (3, 0)
    assert judge(start, p, BATCH, signatures=True, sig_ok=lambda row, pub: row[0] != 1)[:2] == (5, 1)
    stale = list(p)
    stale[1] = (p[1] + 1) % o.R
    assert judge(start, stale, BATCH, proof_verdict=4)[:2] == (2, 1)
    late = list(p)
    late[NP - 1] = (p[NP - 1] + 1) % o.R
    assert judge(start, late, BATCH)[:2] == (4, NP - 1)
    assert judge(start, late, BATCH, signatures=True, sig_ok=lambda row, pub: False)[:2] == (5, 0)
    late[T0 + 2] = P250
    assert judge(start, late, BATCH, proof_verdict=1)[:2] == (1, T0 + 2)


def test_refused_arguments():
    from zkr_hip import ZkrError
    from zkr_hip import rollup as n
    rec = [[1, 2, BAL, 0], [3, 4, BAL, 0]]
    for depth, records, batch in ((0, rec, 1), (25, rec, 1), (1, rec + rec, 1), (2, rec, 0), (2, [[1, 2, o.R, 0], [3, 4, BAL, 0]], 1),
                                  (2, [[1, 2, BAL, P250], [3, 4, BAL, 0]], 1)):
        signals = [0] * (n_public(batch, depth) if batch and depth else 1)
        if batch and depth:
            signals[tx_base(batch, 0) + 1] = 1
        with pytest.raises(ZkrError) as e:
            n.replay_plan_host(depth, records, [signals], batch)
        assert e.value.code == -5
    with pytest.raises(ValueError):
        n.replay_plan_host(2, rec, [b"\0" * 33], 1)
