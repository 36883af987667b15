"""GPU: one operator step (include/zkr.h zkr_operator_*, csrc/zkr_operator.hip, zkr_hip.rollup.Operator) against the hand-written
loop it stands for -- Ledger.sequence, calculate_witness_batch_from_device, check_device, prove_batch_device, verify_each_device --
and against the sequencer's model (tests/sequencer_model.py): what a good step returns and leaves, what a refused step leaves
(nothing), how it nests in a caller's checkpoint, its limits and the edge of a fused group.  RollupCircuit(2, 3), five accounts."""
import pytest

from sequencer_model import NOT_REACHED, Model, keypair, signed_row

pytestmark = pytest.mark.gpu

DEPTH, BATCH, ACCOUNTS = 3, 2, 5
RS, SS = [5, 6, 7, 8], [9, 10, 11, 12]


class _Queue:
    """Rows whose nonces follow the transactions the builder expects to be accepted."""

    def __init__(self, n_accounts=ACCOUNTS):
        self.nonce, self.rows = [0] * n_accounts, []

    def tx(self, frm, to, amount=10, fee=1):
        self.nonce[frm] += 1
        self.rows.append(signed_row(frm, to, amount, fee, self.nonce[frm]))
        return self


def _eight():
    """The queue of tests/test_gpu_sequencer.py::test_from_a_queue_to_verified_proofs_on_the_device."""
    return _Queue().tx(0, 1).tx(1, 0).tx(2, 2).tx(3, 4).tx(4, 3).tx(0, 4).tx(0, 2).tx(3, 2)


def _deposits():
    return [(i, keypair(i)[1], 1000, 0) for i in range(ACCOUNTS)]


def _ledger(depth=DEPTH):
    from zkr_hip import rollup as n
    ledger = n.Ledger(depth)
    ledger.deposit(_deposits())
    return ledger


def _state(ledger):
    return {"root": ledger.root, "info": ledger.info(), "records": ledger.records(), "tree": bytes(ledger.tree().cpu().numpy().tobytes())}


def _loop(env, ledger, rows, rs=None, ss=None, check=True):
    """INTEGRATION.md section 6.1, call for call.  -> statuses, consumed, proofs, the public signals of every witness."""
    import torch
    c = env["circuit"]
    status, inputs, consumed = ledger.sequence(rows, BATCH)
    stream = torch.cuda.current_stream().cuda_stream
    wit = c.calculate_witness_batch_from_device(inputs, stream=stream)
    ptrs = [wit[i].data_ptr() for i in range(len(wit))]
    if check:
        ok, _ = env["system"].check_device(ptrs, stream=stream)
        assert ok is True
    proofs = env["key"].prove_batch_device(ptrs, rs, ss)
    if check:
        assert env["vk"].verify_each_device(proofs, ptrs) == [0] * len(proofs)
    publics = [c.public_signals(bytes(wit[b].cpu().numpy().tobytes())) for b in range(len(wit))]
    return {"status": status, "consumed": consumed, "proofs": proofs, "publics": publics}


@pytest.fixture(scope="module")
def env():
    import zkr_hip
    from zkr_hip import rollup as n
    c = n.RollupCircuit(BATCH, DEPTH)
    r1cs = c.r1cs()
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=[2, 3, 5, 7, 11])
    e = {"circuit": c, "r1cs": r1cs, "key": key, "vk_bin": vk_bin, "system": zkr_hip.ConstraintSystem.load(r1cs), "vk": zkr_hip.VerifyingKey(vk_bin)}
    yield e
    e["system"].close(), e["vk"].close(), key.close()


@pytest.fixture(scope="module")
def looped(env):
    """Ledger X through the hand-written loop with fixed blinding: computed once, read by the cases below, never changed."""
    ledger = _ledger()
    out = _loop(env, ledger, _eight().rows, RS, SS)
    assert out["status"] == [0] * 8 and out["consumed"] == 8 and len(out["proofs"]) == 4
    out["state"] = _state(ledger)
    ledger.close()
    return out


def test_the_step_equals_the_loop(env, looped):
    from zkr_hip import rollup as n
    ledger = _ledger()
    with n.Operator(ledger, env["key"], env["system"], env["vk"], batch=BATCH) as op:
        assert op.info() == {"batch": BATCH, "depth": DEPTH, "n_vars": env["circuit"].n_vars, "n_public": env["circuit"].n_public, "max_batches": 256,
                             "device_bytes": 32 * (env["circuit"].n_vars + env["circuit"].n_public - 1)}
        got = op.step(_eight().rows, RS, SS)
        times = op.stage_times()
        assert op.info()["device_bytes"] == 4 * 32 * (env["circuit"].n_vars + env["circuit"].n_public - 1)   # grown to the step
    for k in ("status", "consumed", "proofs", "publics"):
        assert got[k] == looped[k], k
    assert all(p[0] != 0 for p in got["publics"]) and got["publics"][3][0] == ledger.root
    assert _state(ledger) == looped["state"]
    assert ledger.journal_info() == (0, 0)
    assert set(times) == set(n.Operator.STAGES) and all(v > 0 for v in times.values())
    ledger.close()


def test_the_step_without_system_and_vk_gives_the_same_proofs(env, looped):
    from zkr_hip import rollup as n
    ledger = _ledger()
    with n.Operator(ledger, env["key"], batch=BATCH) as op:
        got = op.step(_eight().rows, RS, SS)
        times = op.stage_times()
    assert got["proofs"] == looped["proofs"] and got["publics"] == looped["publics"]
    assert times["check"] == 0 and times["verify"] == 0 and times["prove"] > 0
    assert _state(ledger) == looped["state"]
    ledger.close()


def test_a_mixed_queue_follows_the_model_and_the_next_step_continues(env):
    """A bad signature, a bad nonce and a tail that fills no whole batch; then the rest of the queue with two more transactions."""
    from zkr_hip import rollup as n
    ledger, model = _ledger(), Model(DEPTH)
    for r in _deposits():
        model.deposit(*r)
    rows = [signed_row(0, 1, 10, 1, 1), signed_row(1, 2, 10, 1, 1, signer=3), signed_row(3, 4, 10, 1, 7), signed_row(2, 3, 10, 1, 1),
            signed_row(4, 0, 10, 1, 1)]
    with n.Operator(ledger, env["key"], env["system"], env["vk"], batch=BATCH) as op:
        got = op.step(rows)
        want_status, want_inputs, want_consumed, _ = model.sequence(rows, BATCH)
        assert want_status == [0, 10, 8, 0, NOT_REACHED] and want_consumed == 4   # three accepted: one batch, a tail of one
        assert got["status"] == want_status and got["consumed"] == want_consumed and len(got["proofs"]) == len(want_inputs) == 1
        assert got["publics"][0][1:] == want_inputs[0] and got["publics"][0][0] == model.tree.root == ledger.root
        assert ledger.records() == model.records()
        rows2 = rows[got["consumed"]:] + [signed_row(3, 1, 10, 1, 1), signed_row(0, 2, 10, 1, 2)]
        got2 = op.step(rows2)
        want_status, want_inputs, want_consumed, _ = model.sequence(rows2, BATCH)
        assert want_status == [0, 0, NOT_REACHED] and want_consumed == 2 and len(want_inputs) == 1   # the old tail found its batch
        assert got2["status"] == want_status and got2["consumed"] == want_consumed and len(got2["proofs"]) == 1
        assert got2["publics"][0][1:] == want_inputs[0] and got2["publics"][0][0] == model.tree.root == ledger.root
    assert ledger.records() == model.records() and ledger.info()["applied"] == 4 and ledger.info()["batches"] == 2
    assert ledger.audit() is None and ledger.journal_info() == (0, 0)
    ledger.close()


def test_one_accepted_transaction_fills_no_batch(env):
    from zkr_hip import rollup as n
    ledger = _ledger()
    before = _state(ledger)
    with n.Operator(ledger, env["key"], env["system"], None, batch=BATCH) as op:
        got = op.step([signed_row(0, 1, 10, 1, 1)])
        assert got == {"status": [NOT_REACHED], "consumed": 0, "proofs": [], "publics": []}
        assert op.step([]) == {"status": [], "consumed": 0, "proofs": [], "publics": []}
    assert _state(ledger) == before and ledger.journal_info() == (0, 0)
    ledger.close()


def test_a_rejected_proof_rolls_the_ledger_back(env, looped):
    """The operator's verifying key comes from another setup of the same circuit: every proof is refused, nothing may move."""
    import zkr_hip
    from zkr_hip import rollup as n
    other_key, other_vk_bin = zkr_hip.ProvingKey.setup_r1cs(env["r1cs"], toxic=[3, 5, 7, 11, 13])
    other_key.close()
    ledger = _ledger()
    before = _state(ledger)
    with zkr_hip.VerifyingKey(other_vk_bin) as other_vk, n.Operator(ledger, env["key"], env["system"], other_vk, batch=BATCH) as op:
        with pytest.raises(zkr_hip.ZkrError) as e:
            op.step(_eight().rows, RS, SS)
        assert e.value.code == -2 and "batch 0: proof rejected by the verifying key (verdict 4)" in str(e.value)
    assert _state(ledger) == before and ledger.audit() is None and ledger.journal_info() == (0, 0)
    with n.Operator(ledger, env["key"], env["system"], env["vk"], batch=BATCH) as op:   # the SAME ledger, a good operator
        got = op.step(_eight().rows, RS, SS)
    assert got["proofs"] == looped["proofs"] and _state(ledger) == looped["state"]
    ledger.close()


def test_a_step_nests_in_the_callers_checkpoint(env, looped):
    from zkr_hip import rollup as n
    ledger = _ledger()
    before = _state(ledger)
    cp = ledger.checkpoint()
    with n.Operator(ledger, env["key"], batch=BATCH) as op:
        got = op.step(_eight().rows, RS, SS)
    assert got["proofs"] == looped["proofs"] and _state(ledger) == looped["state"]
    opened, nodes = ledger.journal_info()
    assert opened == 1 and nodes > 0          # the step's own checkpoint is gone, the caller's still records
    ledger.rollback(cp)
    assert _state(ledger) == before and ledger.audit() is None
    ledger.release(cp)
    assert ledger.journal_info() == (0, 0)
    ledger.close()


def test_limits_and_growing_buffers(env):
    import zkr_hip
    from zkr_hip import rollup as n
    rows = _eight().tx(1, 3).tx(2, 4).rows      # ten accepted transactions
    rs, ss = [21, 22, 23, 24, 25], [31, 32, 33, 34, 35]
    a, b = _ledger(), _ledger()
    before = _state(a)
    with n.Operator(a, env["key"], batch=BATCH, max_batches=2) as op:
        assert op.info()["max_batches"] == 2
        with pytest.raises(zkr_hip.ZkrError) as e:
            op.step(rows[:8])
        assert e.value.code == -5 and "4 batches" in str(e.value)
        assert _state(a) == before and a.journal_info() == (0, 0)
    with n.Operator(a, env["key"], batch=BATCH) as op:                    # one operator: a step of one batch, then one of four
        first = op.step(rows[:2], rs[:1], ss[:1])
        second = op.step(rows[2:], rs[1:], ss[1:])
    with n.Operator(b, env["key"], batch=BATCH) as op:
        want_first = op.step(rows[:2], rs[:1], ss[:1])
    with n.Operator(b, env["key"], batch=BATCH) as op:                    # a fresh operator: its buffers start at the size of the step
        want_second = op.step(rows[2:], rs[1:], ss[1:])
    assert first == want_first and second == want_second and len(second["proofs"]) == 4
    assert _state(a) == _state(b)
    a.close(), b.close()


def test_the_edge_of_a_fused_group(env):
    """fuse() + 1 batches in one step: two fused groups, the second partial.  The proofs are prove_batch_device's."""
    from zkr_hip import rollup as n
    nb = env["key"].fuse() + 1
    q = _Queue()
    for k in range(2 * nb):
        q.tx(k % ACCOUNTS, (k + 1 + k // ACCOUNTS % 3) % ACCOUNTS, amount=1 + k % 3)
    rs, ss = [100 + k for k in range(nb)], [200 + k for k in range(nb)]
    a, b = _ledger(), _ledger()
    want = _loop(env, a, q.rows, rs, ss, check=False)
    assert want["status"] == [0] * (2 * nb) and len(want["proofs"]) == nb
    with n.Operator(b, env["key"], batch=BATCH) as op:
        got = op.step(q.rows, rs, ss)
    for k in ("status", "consumed", "proofs", "publics"):
        assert got[k] == want[k], k
    assert _state(a) == _state(b)
    a.close(), b.close()


def test_mismatched_handles_are_refused_at_construction(env):
    import zkr_hip
    from zkr_hip import rollup as n
    ledger = _ledger()
    deep = _ledger(4)
    with pytest.raises(zkr_hip.ZkrError) as e:
        n.Operator(deep, env["key"], batch=BATCH)
    assert e.value.code == -5 and "BatchProcessTx(2, 4)" in str(e.value) and "nVars" in str(e.value)
    small = n.RollupCircuit(1, DEPTH)
    small_key, small_vk_bin = zkr_hip.ProvingKey.setup_r1cs(small.r1cs(), toxic=[2, 3, 5, 7, 11])
    small_key.close()
    cs = zkr_hip.ConstraintSystem.load(small.r1cs())
    with pytest.raises(zkr_hip.ZkrError) as e:
        n.Operator(ledger, env["key"], cs, batch=BATCH)
    assert e.value.code == -5 and "constraint system is not the key's" in str(e.value) and "nVars" in str(e.value)
    cs.close()
    with zkr_hip.VerifyingKey(small_vk_bin) as vk:
        assert vk.n_public != env["circuit"].n_public
        with pytest.raises(zkr_hip.ZkrError) as e:
            n.Operator(ledger, env["key"], env["system"], vk, batch=BATCH)
        assert e.value.code == -5 and "verifying key has nPublic=%d" % vk.n_public in str(e.value)
    with pytest.raises(zkr_hip.ZkrError) as e:        # the batch is part of the geometry as well
        n.Operator(ledger, env["key"], batch=1)
    assert e.value.code == -5
    assert ledger.journal_info() == (0, 0)
    ledger.close(), deep.close()
