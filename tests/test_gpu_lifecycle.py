"""GPU: handles come and go without leaking device memory.  Every handle of the library holds its device buffers, pinned buffers,
events and streams in owners (csrc/zkr_owners.hpp) that free them when the handle is deleted; these four tests are the check that
they do, in the form of the one at the end of tests/test_gpu_shard.py: one warm-up round (what is made once per process is in
place after it), then five rounds of create / use / close, after which free device memory may have fallen by at most 8 MiB.  The
sizes are chosen so that five leaked copies of a handle's largest allocation exceed that."""
import pytest

pytestmark = pytest.mark.gpu

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SLACK = 8 << 20


def _five_rounds_leave_memory_where_it_was(one_round):
    import torch
    one_round()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(5):
        one_round()
    torch.cuda.synchronize()
    lost = free0 - torch.cuda.mem_get_info(0)[0]
    print("device memory lost over five rounds: %.2f MiB" % (lost / 2 ** 20))
    assert lost <= SLACK


def test_ledger_with_book_and_checkpoint():
    """Depth 16: the tree is 4 MiB, the book's key hashes 2 MiB.  Under a checkpoint two storing calls of 16 384 updates each: the
    second one's nodes do not fit the journal's first capacity (1.5 times the first call's), so the journal grows -- to about 4.7
    MiB, from about 2.3.  4 097 withdrawals in one list into a nullifier table of 2^13 slots (room for 2^12): it doubles (the
    list is short because the binding unpacks a call's events in time quadratic in their number).  Then the rollback, and a
    by-key call that builds both tables again."""
    from zkr_hip import rollup as nat
    depth, n = 16, 1 << 15
    pub = lambda i: (i + 1, R - 1 - i)                                # any two field elements: nothing here looks at the curve
    fill = [(i, pub(i), 10 ** 6, 0) for i in range(n)]
    again = [[(i, pub(i), 10 ** 6 + k, 0) for i in range(0, n, 2)] for k in (1, 2)]
    withdrawals = [pub(i) + (10 ** 9 + i,) for i in range((1 << 12) + 1)]

    def one_round():
        led = nat.Ledger(depth)
        led.deposit(fill)
        led.open_book(nullifier_cap_log2=13, salt=0x5A4B00B00C5EED01)
        root = led.root
        cp = led.checkpoint()
        led.deposit(again[0])
        first = led.journal_info()[1]
        led.deposit(again[1])
        assert led.journal_info() == (1, 2 * first) and first > n    # the leaves and their parents at least
        assert led.book_info()["nullifier_capacity"] == 1 << 13
        verdicts, _ = led.withdraw_calls(withdrawals, [1] * len(withdrawals))
        assert set(verdicts) == {0}
        assert led.book_info()["nullifier_capacity"] == 1 << 14 and led.book_info()["nullifiers"] == len(withdrawals)
        assert led.root != root
        led.rollback(cp)
        assert led.root == root and led.journal_info() == (1, 0)     # the checkpoint stays open after a rollback
        led.release(cp)
        assert led.index_of([pub(5), (1, 1)]) == [5, None] and led.nullifiers_used([10 ** 9]) == [False]
        assert led.book_info()["nullifiers"] == 0 and led.audit() is None
        led.close()

    _five_rounds_leave_memory_where_it_was(one_round)


def test_constraint_system_load_check_close():
    """65 528 constraints (a domain of 2^16) of two A terms, one B term and one C term: the coefficients of A are 4 MiB on the
    device.  Every signal is 1 and every constraint reads (1 + 1) x 1 = 2 x 1."""
    import zkr_hip
    n_vars, n_public = 1 << 16, 7
    rows = [[[(i % n_vars, 1), ((i + 1) % n_vars, 1)], [((3 * i + 2) % n_vars, 1)], [((5 * i + 3) % n_vars, 2)]] for i in range(n_vars - n_public - 1)]
    r1cs = zkr_hip.binarify_r1cs(dict(nVars=n_vars, nPublic=n_public, constraints=rows))
    witness = (1).to_bytes(32, "little") * n_vars
    clean = {"violated": 0, "first": None, "one_ok": True}

    def one_round():
        cs = zkr_hip.ConstraintSystem.load(r1cs)
        assert cs.info()["nConstraints"] == len(rows) and cs.info()["nnzA"] == 2 * len(rows)
        assert cs.check([witness, witness]) == (True, [clean, clean])
        cs.close()

    _five_rounds_leave_memory_where_it_was(one_round)


def test_verifying_key_on_the_device():
    """73 public signals: a batch of n proofs keeps 2 336 n bytes of signals on the device, 2.3 MiB at 1 024.  256 proofs first, so
    that the per-batch buffers are freed and made again for the larger batch."""
    import zkr_hip
    p = 73
    key, wb, aux = zkr_hip.ProvingKey.synth(7, p, 0x5A4B0001, 0x5A4B00FF)
    vkb = key.synth_vk(aux)
    proof = key.prove(wb, 0x1234567890ABCDEF, 0x0FEDCBA987654321)
    key.close()
    pub = [int.from_bytes(wb[32 * i:32 * i + 32], "little") for i in range(1, p + 1)]
    assert zkr_hip.verify(vkb, proof, pub)

    def one_round():
        vk = zkr_hip.VerifyingKey(vkb)
        for n in (256, 1024):
            assert vk.verify_each([proof] * n, [pub] * n) == [0] * n and vk.all_valid
        vk.close()

    _five_rounds_leave_memory_where_it_was(one_round)


def test_eval_tables_then_drop():
    """A key of 2^12 loaded from websnark bytes proves through the coefficient form; with its side tables derived -- 4 096 points at
    22 window levels are 5.5 MiB for E' alone -- through the evaluation form, and the two proofs are the same bytes."""
    import groth16 as g
    import zkr_hip
    circ = g.synth_circuit(1 << 12, 7, 0x5A4B0001)
    r1cs = zkr_hip.binarify_r1cs(dict(nVars=circ["nVars"], nPublic=circ["nPublic"], constraints=[[list(lc) for lc in row] for row in circ["rows"]]))
    pkb, _ = zkr_hip.setup_r1cs_websnark(r1cs, toxic=[2, 3, 5, 7, 11])
    key = zkr_hip.ProvingKey.load_websnark(pkb)
    wb = g.binarify_witness(circ["witness"])
    r, s = 0x1234567890ABCDEF, 0x0FEDCBA987654321
    want = key.prove(wb, r, s)
    assert key.h_form() == {"form": "coefficients", "retries": 0}

    def one_round():
        assert key.eval_tables(r1cs) is True and key.h_form()["form"] == "evaluation"
        assert key.prove(wb, r, s) == want
        key.drop_eval_tables()
        assert key.h_form()["form"] == "coefficients"
        assert key.prove(wb, r, s) == want

    _five_rounds_leave_memory_where_it_was(one_round)
    assert key.h_form()["retries"] == 0
    key.close()
