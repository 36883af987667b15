"""GPU: proofs with H in evaluation form (csrc/eval_h.hpp; include/zkr.h zkr_key_h_form) are the bytes of the coefficient form.

Keys come from zkr_setup_r1cs with injected toxic scalars, so every proof has three references: the closed form from the toxic
scalars, the C oracle on the websnark rendering of the same setup, and the verifier.  key.h_form() is where a key says which form
its own proofs take (info() describes the arena and stays equal between a key and its replicas)."""
import random

import pytest

import coracle
import groth16 as g
from groth16 import R

pytestmark = pytest.mark.gpu

TOX = ("t", "alfa", "beta", "gamma", "delta")


def _setup(circ, side_tables=True):
    import zkr_hip
    tox = g.toxic_from_seed(0x5A4B00FF)
    r1cs = zkr_hip.binarify_r1cs(dict(nVars=circ["nVars"], nPublic=circ["nPublic"], constraints=[[list(lc) for lc in row] for row in circ["rows"]]))
    toxic = [tox[k] for k in TOX]
    key, vk = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=toxic, side_tables=side_tables)
    pkb, _ = zkr_hip.setup_r1cs_websnark(r1cs, toxic=toxic)  # the same setup as the bytes the oracle reads
    return dict(circ=circ, tox=tox, key=key, vk=vk, pkb=pkb, w=circ["witness"], wb=g.binarify_witness(circ["witness"]))


def _closed(c, r, s):
    return g.proof_bytes(g.proof_from_toxic(c["circ"], c["tox"], c["w"], r, s))


def _device(witnesses):
    import torch
    return [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in witnesses]


@pytest.fixture(scope="module", params=[7, 12], ids=["one_pass", "two_passes"])
def sized(request):
    """Domain 2^7: every transform is one pass; 2^12: the smallest with two (a strided pass in front of the tile of 2048)."""
    log_m = request.param
    c = _setup(g.synth_circuit(1 << log_m, 7, 0x5A4B0001))
    c["log_m"] = log_m
    yield c
    c["key"].close()


def _five(c, bad_third):
    """Five witnesses of the circuit (other free values each) with their blinding; bad_third: the third one is random field
    elements behind w_0 = 1 and satisfies nothing."""
    import zkr_hip
    rnd = random.Random(31 * c["log_m"] + bad_third)
    wits = [c["wb"]] + [zkr_hip.synth_witness(c["log_m"], 7, 0x5A4B0001, 900 + i) for i in range(1, 5)]
    if bad_third:
        wits[2] = g.binarify_witness([1] + [rnd.randrange(R) for _ in range(len(c["w"]) - 1)])
    rs, ss = [rnd.randrange(R) for _ in wits], [rnd.randrange(R) for _ in wits]
    return wits, rs, ss


def test_single_proof_is_the_closed_form_and_the_oracles(sized):
    c, key = sized, sized["key"]
    assert key.h_form()["form"] == "evaluation" and key.info()["domainSize"] == 1 << c["log_m"]
    before = key.h_form()["retries"]
    r, s = 0x1234567890ABCDEF, 0x0FEDCBA987654321
    proof = key.prove(c["wb"], r, s)
    assert proof == _closed(c, r, s) == coracle.prove(c["pkb"], c["wb"], r, s)
    assert key.h_form()["retries"] == before  # a satisfying witness is proved once


def test_pipelined_batch_of_five(sized):
    """Single proofs two in flight (the unfused submit / collect loop: fused batches keep the coefficient form)."""
    import torch
    c, key = sized, sized["key"]
    wits, rs, ss = _five(c, False)
    before = key.h_form()["retries"]
    dev = _device(wits)
    got = key.prove_batch_device([t.data_ptr() for t in dev], rs, ss, stream=torch.cuda.current_stream().cuda_stream, depth=2)
    assert got == [coracle.prove(c["pkb"], wb, r, s) for wb, r, s in zip(wits, rs, ss)]
    assert got[0] == _closed(c, rs[0], ss[0])
    assert key.h_form()["retries"] == before


def test_unsatisfying_witness_is_proved_again_in_its_place(sized):
    import torch
    c, key = sized, sized["key"]
    wits, rs, ss = _five(c, True)
    before = key.h_form()["retries"]
    dev = _device(wits)
    got = key.prove_batch_device([t.data_ptr() for t in dev], rs, ss, stream=torch.cuda.current_stream().cuda_stream, depth=2)
    want = [coracle.prove(c["pkb"], wb, r, s) for wb, r, s in zip(wits, rs, ss)]
    assert got == want and len(set(got)) == 5  # all five, in the caller's order
    assert key.h_form()["retries"] == before + 1
    # ... and alone, from a host buffer
    assert key.prove(wits[2], rs[2], ss[2]) == want[2] and key.h_form()["retries"] == before + 2
    assert key.prove(wits[3], rs[3], ss[3]) == want[3] and key.h_form()["retries"] == before + 2


def _public_in_c():
    """Domain 2^7, three public signals; every third constraint also carries a public signal on its C side, so the folded C table
    has points for public signals, which the plain C query has none for."""
    rnd = random.Random(0x5A4B0300)
    p, m = 3, 128
    w = [1] + [rnd.randrange(1, R) for _ in range(p)]
    rows = []
    for row in range(m - p - 1):
        n = len(w)
        A = sorted({n - 1: 1, rnd.randrange(n): rnd.randrange(1, R)}.items())
        B = [(rnd.randrange(n), rnd.randrange(1, R))]
        val = sum(cf * w[s] for s, cf in A) * sum(cf * w[s] for s, cf in B) % R
        C = []
        if row % 3 == 0:
            pub, cf = 1 + rnd.randrange(p), rnd.randrange(1, R)
            C.append((pub, cf))
            val = (val - cf * w[pub]) % R
        rows.append((A, B, C + [(n, 1)]))
        w.append(val)
    circ = dict(nVars=len(w), nPublic=p, nConstraints=len(rows), domainSize=m, rows=rows, witness=w)
    assert g.check_r1cs(circ)
    return circ


def test_public_signal_in_c():
    import zkr_hip
    c = _setup(_public_in_c())
    key = c["key"]
    assert key.h_form()["form"] == "evaluation"
    r, s = 77, 99
    proof = key.prove(c["wb"], r, s)
    assert proof == _closed(c, r, s) == coracle.prove(c["pkb"], c["wb"], r, s)
    assert zkr_hip.verify(c["vk"], proof, c["w"][1:4]) and key.h_form()["retries"] == 0
    key.close()


def test_c_and_h_reduced_apart():
    """100 signals under a domain of 2^8 (tests/layout_cases.py): C's window follows the signals, H's the domain, so C' and E'
    -- which take the plans of C and H -- are reduced by a chain each."""
    from layout_cases import few_signals_many_constraints
    lc = few_signals_many_constraints()
    c = _setup(lc["circ"])
    key = c["key"]
    win = key.windows()
    assert key.h_form()["form"] == "evaluation" and win["C"][0] == 7 and win["H"][0] == 8
    r, s = 5, 7
    assert key.prove(c["wb"], r, s) == _closed(c, r, s) == coracle.prove(lc["pkb"], c["wb"], r, s)  # the oracle on the ORACLE's setup of the circuit
    rnd = random.Random(8)
    bad = g.binarify_witness([1] + [rnd.randrange(R) for _ in range(99)])
    assert key.prove(bad, r, s) == coracle.prove(lc["pkb"], bad, r, s) and key.h_form()["retries"] == 1
    key.close()


def test_refused_side_tables_leave_the_coefficient_form(sized):
    c = _setup(sized["circ"], side_tables=False)
    key = c["key"]
    assert key.h_form() == {"form": "coefficients", "retries": 0}
    r, s = 11, 13
    assert key.prove(c["wb"], r, s) == sized["key"].prove(c["wb"], r, s) == _closed(c, r, s)
    key.close()


def test_contributed_key_has_no_side_tables(sized):
    """A delta contribution changes the points of C and H: the key it returns is built from the arena alone and proves through the
    coefficient form, under the contributed verifying key."""
    import zkr_hip
    c, key = sized, sized["key"]
    k2, rec = key.contribute(0x1234567)
    assert key.h_form()["form"] == "evaluation" and k2.h_form() == {"form": "coefficients", "retries": 0}
    proof = k2.prove(c["wb"], 3, 4)
    pub = c["w"][1:8]
    assert zkr_hip.verify(zkr_hip.vk_contribute(c["vk"], rec), proof, pub) and not zkr_hip.verify(c["vk"], proof, pub)
    k2.close()
