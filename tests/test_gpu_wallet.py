"""GPU: keys, signatures and withdraw witnesses in bulk (csrc/zkr_wallet.hip) against the host calls they stand in for, item by item
and bit for bit, at the sizes where a one-thread-per-item kernel can go wrong: one item, and 70 (one wavefront and a partial one)."""
import pytest

import wallet_cases as wc
import zkr_hip
from zkr_hip import rollup as n

pytestmark = pytest.mark.gpu
R = n.SNARK_FIELD_SIZE


@pytest.fixture(scope="module")
def host():
    """What the host calls give for the case list, computed once."""
    keys = wc.keys()
    return {"keys": keys, "formatted": [n.format_priv_key(k) for k in keys], "pubs": [n.gen_public_key(k) for k in keys]}


def test_format_and_pubkey_batches_equal_the_host_calls_and_the_oracle(host):
    keys = list(host["keys"])
    assert len(keys) == 70
    lens = [wc.text_len(k) for k in keys[:8]]
    assert 64 in lens and 63 in lens and min(lens) <= 62
    assert n.format_priv_key_batch(keys) == host["formatted"] == list(wc.oracle_formatted())
    assert n.gen_public_key_batch(keys) == host["pubs"] == list(wc.oracle_pubs())
    for one in (keys[2], keys[7]):   # r - 1, and the key with the short text
        i = keys.index(one)
        assert n.format_priv_key_batch([one]) == [host["formatted"][i]] and n.gen_public_key_batch([one]) == [host["pubs"][i]]


@pytest.mark.parametrize("arity,count", [(5, 70), (1, 3), (8, 3)])
def test_sign_batch_equals_sign_and_verifies(host, arity, count):
    keys = list(host["keys"])
    if count < len(keys):
        keys = keys[5:5 + count]     # the three text lengths
    first = host["keys"].index(keys[0])
    msgs = [list(m) for m in wc.messages(arity)[first:first + len(keys)]]
    pubs = host["pubs"][first:first + len(keys)]
    sigs = n.sign_batch(keys, msgs)
    assert sigs == [n.sign(k, m) for k, m in zip(keys, msgs)]
    assert n.verify_batch(msgs, sigs, pubs) == [True] * len(keys)
    changed = [m[:-1] + [(m[-1] + 1) % R] for m in msgs]
    assert n.verify_batch(changed, sigs, pubs) == [False] * len(keys)


def test_a_ledger_takes_a_queue_signed_by_sign_batch(host):
    keys = list(host["keys"][3:7])
    pubs = n.gen_public_key_batch(keys)
    ledger = n.Ledger(3)
    ledger.deposit([(i, pubs[i], 10 ** 6, 0) for i in range(4)])
    txs = [(0, 1, 10, 1, 1), (1, 2, 20, 1, 1), (2, 3, 30, 1, 1), (0, 3, 40, 1, 2)]   # from to amount fee nonce
    sigs = n.sign_batch([keys[t[0]] for t in txs], [list(t) for t in txs])
    status, inputs, consumed = ledger.sequence([n.tx_row(*t, s) for t, s in zip(txs, sigs)], 2)
    assert status == [0, 0, 0, 0] and consumed == 4 and inputs.shape[0] == 2
    assert ledger.info()["batches"] == 2 and ledger.info()["applied"] == 4


@pytest.fixture(scope="module")
def withdraw(host):
    c = n.WithdrawCircuit()
    cases = [{"privateKey": host["formatted"][i], "nullifier": wc.nullifiers()[i]} for i in range(9)]   # a fused group of 8 and one more
    cases[0]["nullifier"], cases[1]["nullifier"] = 0, R - 1
    return {"circuit": c, "cases": cases, "want": [c.calculate_witness(x) for x in cases], "pubs": host["pubs"][:9]}


def _rows(t):
    return [bytes(r) for r in t.cpu().numpy()]


def test_withdraw_witnesses_equal_the_host_builder_and_prove(withdraw):
    import torch
    c, cases, want = withdraw["circuit"], withdraw["cases"], withdraw["want"]
    dev = c.calculate_witness_batch_device(cases)
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (9, c.n_vars * 32)
    assert _rows(dev) == want
    assert _rows(c.calculate_witness_batch_device(cases[4:5])) == want[4:5]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = c.calculate_witness_batch_device(cases, stream=side.cuda_stream)
    assert _rows(other) == want
    # the chain behind it: check, prove, verify, all from the witnesses where they lie
    r1cs = c.r1cs()
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(r1cs)
    ptrs = [dev[i].data_ptr() for i in range(9)]
    cs = zkr_hip.ConstraintSystem.load(r1cs)
    ok, reports = cs.check_device(ptrs)
    assert ok and all(r["violated"] == 0 and r["one_ok"] for r in reports)
    proofs = key.prove_batch_device(ptrs)
    vk = zkr_hip.VerifyingKey(vk_bin)
    assert vk.verify_each_device(proofs, ptrs) == [0] * 9 and vk.all_valid
    for row, case, pub in zip(_rows(dev), cases, withdraw["pubs"]):
        assert tuple(c.public_signals(row)) == (pub[0], pub[1], case["nullifier"])
    assert vk.verify_each(proofs, [c.public_signals(w) for w in want]) == [0] * 9
    cs.close()
    vk.close()


def test_withdraw_refusals_leave_the_next_call_right(withdraw):
    c, cases, want = withdraw["circuit"], withdraw["cases"], withdraw["want"]
    bad = [dict(x) for x in cases]
    bad[5]["privateKey"] = 1 << 253
    with pytest.raises(zkr_hip.ZkrError) as e:
        c.calculate_witness_batch_device(bad)
    assert e.value.code == -7 and "witness 5" in str(e.value) and "private key fits 253 bits" in str(e.value)
    bad = [dict(x) for x in cases]
    bad[3]["nullifier"] = R
    with pytest.raises(zkr_hip.ZkrError) as e:
        c.calculate_witness_batch_device(bad)
    assert e.value.code == -5 and "witness 3" in str(e.value)
    assert _rows(c.calculate_witness_batch_device(cases)) == want
