"""GPU: the ledger's one storing path (csrc/zkr_sequencer.hip stage_updates / store_updates) seen through its three callers.
`sequence`, `replay` and `deposit` reach the same records by three routes; under an open checkpoint each must leave the same
tree, a sound audit, and a journal that puts the tree back byte for byte.  And the prefix case of a replay that stops early: the
tables of the stored prefix, over the value rows of the longer list that was hashed."""
import copy

import pytest

import rollup as o
from replay_model import publish, tx_base
from sequencer_model import le
from test_gpu_sequencer import _pair, _Queue

pytestmark = pytest.mark.gpu

DEPTH, BATCH, ACCOUNTS = 3, 2, 6


def _tree(ledger):
    return ledger.tree().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def chain():
    """Two batches; the second writes the leaves the first one wrote, so "holds the last version of its node" differs between
    the list of both batches and its prefix."""
    q = _Queue(ACCOUNTS)
    q.tx(0, 1), q.tx(2, 3), q.tx(1, 0), q.tx(3, 2)
    _, model = _pair(DEPTH, ACCOUNTS)
    return {"rows": q.rows, "publics": publish(copy.deepcopy(model), q.rows, BATCH)}


def _sequenced(rows):
    """A ledger that took `rows` through sequence under an open checkpoint -> (ledger, checkpoint, tree before, inputs)."""
    a, _ = _pair(DEPTH, ACCOUNTS)
    cp, before = a.checkpoint(), _tree(a)
    status, inputs, consumed = a.sequence(rows, BATCH)
    assert status == [0] * len(rows) and consumed == len(rows)
    return a, cp, before, inputs.cpu().numpy()


def test_the_three_callers_store_alike(chain):
    rows, publics = chain["rows"], chain["publics"]
    a, cp_a, before_a, inputs = _sequenced(rows)
    assert [inputs[b].tobytes() for b in range(2)] == [le(p[1:]) for p in publics]        # A published the model's signals
    b, _ = _pair(DEPTH, ACCOUNTS)
    cp_b, before_b = b.checkpoint(), _tree(b)
    assert b.replay(publics, BATCH) == ([0, 0], [0, 0], 2)
    c, _ = _pair(DEPTH, ACCOUNTS)
    cp_c, before_c = c.checkpoint(), _tree(c)
    c.deposit([(i, (r[0], r[1]), r[2], r[3]) for i, r in enumerate(a.records())])         # the resulting records as overwrites
    assert before_a == before_b == before_c
    assert _tree(a) == _tree(b) == _tree(c) != before_a
    assert a.records() == b.records() == c.records()
    assert a.audit() is None and b.audit() is None and c.audit() is None
    assert a.journal_info() == b.journal_info() and a.journal_info()[1] > 0               # they stored the same list
    assert c.journal_info()[1] > 0
    for ledger, cp, before in ((a, cp_a, before_a), (b, cp_b, before_b), (c, cp_c, before_c)):
        ledger.rollback(cp)
        assert _tree(ledger) == before
        assert ledger.audit() is None and ledger.info()["applied"] == 0


def test_a_replay_that_stops_early_stores_the_prefix(chain):
    at = 1 + (17 + DEPTH) * BATCH + 1 * DEPTH + 1                     # txRecipientPathElements[1][1] of batch 1
    spoiled = [list(p) for p in chain["publics"]]
    spoiled[1][at] = (spoiled[1][at] + 1) % o.R
    touched = lambda p: {p[tx_base(BATCH, k) + j] for k in range(BATCH) for j in (0, 1)}
    assert touched(spoiled[0]) == touched(spoiled[1])                # stale tables would name batch 1's nodes as the last versions
    b, _ = _pair(DEPTH, ACCOUNTS)
    b.checkpoint()
    assert b.replay(spoiled, BATCH) == ([0, 4], [0, at], 1)
    d, _, _, _ = _sequenced(chain["rows"][:BATCH])
    assert _tree(b) == _tree(d)
    assert b.journal_info() == d.journal_info() and b.journal_info()[1] > 0
    assert b.records() == d.records() and b.audit() is None
    assert b.info() == d.info() == {"depth": DEPTH, "accounts": ACCOUNTS, "applied": BATCH, "batches": 1}
