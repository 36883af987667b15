"""GPU: the Ecdh circuit (zkr_hip.circuit.Ecdh; prover/circuits/ecdh.circom) as a witness program on the device: sharedKey of every
witness equals the bulk ecdh call's and the model's, a failing instance in either piece is reported and zeroed and touches no
other, and three instances go witness -> check -> prove -> verify in device memory."""
import pytest

import crypto_model as m
import wallet_cases as wc

pytestmark = pytest.mark.gpu
R = m.R
N = 65   # two pieces of 64


def _ints(b):
    return [int.from_bytes(b[k:k + 32], "little") for k in range(0, len(b), 32)]


def _rows_bytes(t):
    return [bytes(r) for r in t.cpu().numpy()]


@pytest.fixture(scope="module")
def case():
    """the circuit, its program, and N instances: key t of the case list (unformatted and formatted) with the public key of key t + 1"""
    from zkr_hip import circuit as C
    from zkr_hip import rollup as n
    c = C.Ecdh()
    keys = list(wc.keys())[:N]
    pubs = [n.gen_public_key(k) for k in wc.keys()]
    peers = (pubs[1:] + pubs[:1])[:N]
    rows = [[p[0], p[1], n.format_priv_key(k)] for k, p in zip(keys, peers)]
    return dict(c=c, blob=c.program(), keys=keys, peers=peers, rows=rows)


def test_shared_key_of_every_witness_equals_the_bulk_call_and_failures_stay_contained(case):
    import zkr_hip
    from zkr_hip import rollup as n
    c, rows = case["c"], case["rows"]
    prog = zkr_hip.WitnessProgram(case["blob"], piece=64, statements=c.statements)
    try:
        assert prog.info()["piece"] == 64 and prog.info()["nVars"] == c.n_vars
        clean = _rows_bytes(prog.witness_batch_device(rows))
        shared = [_ints(w[32:64])[0] for w in clean]
        assert shared == n.ecdh_batch(case["keys"], case["peers"])
        for t in (0, 1, 5, 63, 64):
            assert shared[t] == m.ecdh(case["keys"][t], case["peers"][t]), t
            assert clean[t] == zkr_hip.wprog_run_host(case["blob"], rows[t]).witness
        for at, bad, text in ((0, [rows[0][0], rows[0][1], 1 << 253], "private key fits 253 bits"), (64, [1, 1, rows[64][2]], "public key is on the curve")):
            broken = list(rows)
            broken[at] = bad
            with pytest.raises(zkr_hip.ZkrError) as e:
                prog.witness_batch_device(broken)
            assert e.value.code == -7 and str(e.value).endswith("instance %d violates: %s" % (at, text))
            assert [j for j, r in enumerate(e.value.reports) if r[0]] == [at] and e.value.reports[at] == (2, c.statements.index(text))
            got = _rows_bytes(prog.last)
            assert got[at] == bytes(len(got[at])) and got[:at] + got[at + 1:] == clean[:at] + clean[at + 1:]
    finally:
        prog.close()


def test_three_instances_check_prove_and_verify_and_an_altered_shared_key_is_refused(case):
    import torch
    import zkr_hip
    c, rows = case["c"], case["rows"][3:6]
    key, vkb = zkr_hip.ProvingKey.setup_r1cs(c.r1cs(), toxic=[11, 12, 13, 14, 15])
    cs = zkr_hip.ConstraintSystem.load(c.r1cs())
    vk = zkr_hip.VerifyingKey(vkb)
    prog = zkr_hip.WitnessProgram(case["blob"], piece=64, statements=c.statements)
    try:
        assert key.info()["nVars"] == c.n_vars and key.info()["nPublic"] == c.n_public == 3
        wit = prog.witness_batch_device(rows)
        ptrs = [wit[j].data_ptr() for j in range(3)]
        ok, reports = cs.check_device(ptrs)
        assert ok and all(r == {"violated": 0, "first": None, "one_ok": True} for r in reports)
        proofs = key.prove_batch_device(ptrs, rs=[3, 4, 5], ss=[40, 41, 42])
        assert vk.verify_each_device(proofs, ptrs) == [0, 0, 0] and vk.all_valid
        word = wit[1].view(torch.int64)
        word[4 * 1] += 1                     # sharedKey of the second instance, plus one
        torch.cuda.synchronize()
        verdicts = vk.verify_each_device(proofs, ptrs)
        assert verdicts[0] == 0 and verdicts[2] == 0 and verdicts[1] != 0 and not vk.all_valid
        ok, reports = cs.check_device(ptrs)
        assert not ok and [j for j, r in enumerate(reports) if r["violated"]] == [1] and reports[1]["first"] == len(c.constraints) - 1
    finally:
        for h in (prog, vk, cs, key):
            h.close()
