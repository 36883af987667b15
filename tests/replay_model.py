"""The model the replay tests hold zkr_ledger_replay to (tests/test_replay_cpu.py, tests/test_gpu_replay.py): the verdict list
of include/zkr.h applied one batch at a time in Python over tests/sequencer_model.py and oracle/rollup.py (Tree, leaf_hash,
batch_public_signals and the state transition of process_tx_inputs).  Every batch is applied to a copy of the state one
transaction at a time, its full public signal list is derived again from that, and the claimed list is compared with it signal
by signal.  Not a test module."""
import copy

import rollup as o
from sequencer_model import NOT_REACHED, P250, apply_tx, sig_ok_oracle


def n_public(batch, depth):
    return 1 + batch * (18 + 3 * depth)


def tx_base(batch, k):
    """Index of transaction k's txData row among a batch's public signals."""
    return 1 + batch + 8 * k


def publish(model, rows, batch):
    """What an operator whose state is `model` would publish for `rows` (len a multiple of batch): the transactions applied to
    the model as the contract applies them -- no operator rule is looked at -- and the public signals of every batch."""
    assert len(rows) % batch == 0
    out = []
    for b in range(0, len(rows), batch):
        out.append(o.batch_public_signals([apply_tx(model.tree, model.accounts, list(r)) for r in rows[b:b + batch]]))
    return out


def cannot_apply(accounts, signals, batch):
    """Code 1: the offending signal of a batch that cannot be applied to `accounts` (which is moved along, so pass a copy), or
    None.  The lowest signal not below r; else, transaction by transaction: from, to, amount, fee, nonce, the balances."""
    for i, v in enumerate(signals):
        if v >= o.R:
            return i
    for k in range(batch):
        base = tx_base(batch, k)
        frm, to, amount, fee, nonce = signals[base:base + 5]
        if frm not in accounts:
            return base
        if to not in accounts:
            return base + 1
        for j, v in ((2, amount), (3, fee), (4, nonce)):
            if v >= P250:
                return base + j
        if accounts[frm][2] < amount + fee:
            return base + 2
        accounts[frm][2] -= amount + fee
        accounts[frm][3] = nonce
        if accounts[to][2] + amount >= P250:
            return base + 2
        accounts[to][2] += amount
    return None


def judge(model, signals, batch, proof_verdict=0, signatures=False, sig_ok=sig_ok_oracle):
    """-> (verdict, where, the model after the batch or None)."""
    signals = [int(v) for v in signals]
    assert len(signals) == n_public(batch, model.depth)
    bad = cannot_apply(copy.deepcopy(model.accounts), signals, batch)
    if bad is not None:
        return 1, bad, None
    if signals[1] != model.tree.root:
        return 2, 1, None
    if proof_verdict:
        return 3, 0, None
    rows = [signals[tx_base(batch, k):tx_base(batch, k) + 8] for k in range(batch)]
    if signatures:
        for k, row in enumerate(rows):
            if not sig_ok(row, model.accounts[row[0]][:2]):
                return 5, k, None
    after = copy.deepcopy(model)
    derived = o.batch_public_signals([apply_tx(after.tree, after.accounts, row) for row in rows])
    for i, (want, got) in enumerate(zip(derived, signals)):
        if want != got:
            return 4, i, None
    return 0, 0, after


def replay(model, publics, batch, proof_verdicts=None, signatures=False, sig_ok=sig_ok_oracle):
    """-> (verdicts, where, applied).  The model moves to the state after the last batch with verdict 0."""
    verdicts, where = [], []
    for b, signals in enumerate(publics):
        code, at, after = judge(model, signals, batch, proof_verdicts[b] if proof_verdicts else 0, signatures, sig_ok)
        verdicts.append(code), where.append(at)
        if code:
            break
        model.accounts, model.tree = after.accounts, after.tree
    applied = len(verdicts) - (1 if verdicts and verdicts[-1] else 0)
    rest = len(publics) - len(verdicts)
    return verdicts + [NOT_REACHED] * rest, where + [0] * rest, applied
