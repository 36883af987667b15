"""GPU: FUSED groups of a whole key with side tables prove with H in evaluation form (csrc/zkr_prove.hip calc_h_eval with nbat > 1,
csrc/kernels_ntt.hpp eval_unsatisfied_kernel / eval_product_kernel over blockIdx.y), and a group with an unsatisfying witness is
proved again as a whole through the coefficient form (prove_collect).

Keys come from zkr_setup_r1cs with injected toxic scalars, so every proof has the closed form from the toxic scalars and the C oracle
on the websnark rendering of the same setup as references; the oracle is exact for unsatisfying witnesses too.  Domains 2^7 (every
transform is one pass) and 2^12 (the smallest with two): the smallest sizes at which the kernels differ.  A key's pool of witnesses,
their blinding and their oracle proofs are made once per size and shared by the tests.

How a batch call is cut into groups (zkr_prove.hip group_count, capacity 16 at both sizes): up to 8 witnesses are one group, 9..16 two
halves, 17..32 two groups of 9..16.  So 5 and 8 witnesses are one group, key.fuse() witnesses are two groups of 8, key.fuse() + 3 are
groups of 10 and 9, and only a batch of 2 key.fuse() fills a group to its capacity and reaches the slot's last counter word."""
import random

import pytest

import coracle
import groth16 as g
from groth16 import R

pytestmark = pytest.mark.gpu

TOX = ("t", "alfa", "beta", "gamma", "delta")
EVAL, COEF = "evaluation", "coefficients"
POOL = 32


def _r1cs(circ):
    import zkr_hip
    return zkr_hip.binarify_r1cs(dict(nVars=circ["nVars"], nPublic=circ["nPublic"], constraints=[[list(lc) for lc in row] for row in circ["rows"]]))


def _setup(circ):
    import zkr_hip
    tox = g.toxic_from_seed(0x5A4B00FF)
    r1cs = _r1cs(circ)
    toxic = [tox[k] for k in TOX]
    key, vk = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=toxic)
    pkb, _ = zkr_hip.setup_r1cs_websnark(r1cs, toxic=toxic)  # the same setup as the bytes the oracle reads
    return dict(circ=circ, tox=tox, r1cs=r1cs, key=key, vk=vk, pkb=pkb, w=circ["witness"], wb=g.binarify_witness(circ["witness"]))


def _closed(c, r, s):
    return g.proof_bytes(g.proof_from_toxic(c["circ"], c["tox"], c["w"], r, s))


def _device(witnesses):
    import torch
    return [torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() for b in witnesses]


def _prove_device(key, wits, rs, ss):
    """One fused call (no depth) from witnesses resident on the device."""
    import torch
    dev = _device(wits)
    return key.prove_batch_device([t.data_ptr() for t in dev], rs, ss, stream=torch.cuda.current_stream().cuda_stream)


def _bad_witness(n_vars, seed):
    """Random field elements behind w_0 = 1: satisfies nothing."""
    rnd = random.Random(seed)
    return g.binarify_witness([1] + [rnd.randrange(R) for _ in range(n_vars - 1)])


class Pool:
    """POOL witnesses of one synthetic circuit (the circuit's own, then other free values), a blinding pair per position, a bad witness
    per position on demand, and the oracle's proof of either, computed once."""

    def __init__(self, c, log_m):
        import zkr_hip
        rnd = random.Random(0x5A4B0400 + log_m)
        self.c, self.log_m = c, log_m
        self.good = [c["wb"]] + [zkr_hip.synth_witness(log_m, 7, 0x5A4B0001, 900 + i) for i in range(1, POOL)]
        self.rs, self.ss = [rnd.randrange(R) for _ in range(POOL)], [rnd.randrange(R) for _ in range(POOL)]
        self._bad, self._want = {}, {}

    def bad(self, i):
        if i not in self._bad:
            self._bad[i] = _bad_witness(len(self.c["w"]), 7919 * self.log_m + i)
        return self._bad[i]

    def batch(self, n, bad=()):
        """(witnesses, rs, ss, oracle proofs) of positions 0..n-1, the positions in `bad` unsatisfying."""
        wits = [self.bad(i) if i in bad else self.good[i] for i in range(n)]
        want = []
        for i, wb in enumerate(wits):
            k = (i, i in bad)
            if k not in self._want:
                self._want[k] = coracle.prove(self.c["pkb"], wb, self.rs[i], self.ss[i])
            want.append(self._want[k])
        return wits, self.rs[:n], self.ss[:n], want


@pytest.fixture(scope="module", params=[7, 12], ids=["one_pass", "two_passes"])
def sized(request):
    log_m = request.param
    c = _setup(g.synth_circuit(1 << log_m, 7, 0x5A4B0001))
    c["log_m"] = log_m
    c["pool"] = Pool(c, log_m)
    yield c
    c["key"].close()


def _launches(key):
    prof = key.prof()
    return {st: prof[st][1] for st in ("ntt_pass", "combine_h", "spmv_a")}


# ---------------------------------------------------------------- 1. the form is taken
def test_fused_group_runs_four_transforms(sized):
    """One group of satisfying witnesses with the side tables and without: the ntt_pass launches are two run_ntt calls against
    three, of the same passes each; the product stands where the combination stood and the three-side SpMV is still one launch."""
    c, key, pool = sized, sized["key"], sized["pool"]
    assert key.fuse() >= 2
    assert key.h_form()["form"] == EVAL
    before = key.h_form()["retries"]
    n = max(2, key.fuse() // 2)
    wits, rs, ss, want = pool.batch(n)
    key.prof_enable(True)
    try:
        key.prof_reset()
        got_eval = _prove_device(key, wits, rs, ss)
        l_eval, retries = _launches(key), key.h_form()["retries"]
        key.drop_eval_tables()
        assert key.h_form()["form"] == COEF
        key.prof_reset()
        got_coef = _prove_device(key, wits, rs, ss)
        l_coef = _launches(key)
    finally:
        key.prof_enable(False)
        key.prof_reset()
        rebuilt = key.eval_tables(c["r1cs"])  # the module's key goes on with its tables (derived from its points: the same bytes)
    assert rebuilt is True and key.h_form()["form"] == EVAL
    print("launches: evaluation form", l_eval, "coefficient form", l_coef)
    assert l_coef["ntt_pass"] > 0 and 3 * l_eval["ntt_pass"] == 2 * l_coef["ntt_pass"]
    assert l_eval["combine_h"] == l_coef["combine_h"] == 1 and l_eval["spmv_a"] == l_coef["spmv_a"] == 1
    assert got_eval == got_coef == want
    assert got_eval[0] == _closed(c, rs[0], ss[0])
    assert retries == before  # satisfying witnesses are proved once


# ---------------------------------------------------------------- 2. a bad witness inside a group
def test_bad_witness_inside_a_group(sized):
    c, key, pool = sized, sized["key"], sized["pool"]
    assert key.fuse() >= 2
    before = key.h_form()["retries"]
    wits, rs, ss, want = pool.batch(5, bad=(2,))
    got = _prove_device(key, wits, rs, ss)
    assert got == want and len(set(got)) == 5  # all five, in the caller's order
    assert key.h_form()["retries"] == before + 1  # the witnesses that failed, not the size of the group that went again
    wits, rs, ss, want = pool.batch(5, bad=(1, 4))
    got = _prove_device(key, wits, rs, ss)
    assert got == want and len(set(got)) == 5
    assert key.h_form()["retries"] == before + 3


# ---------------------------------------------------------------- 3. capacity edges
def test_batch_of_the_capacity_with_the_last_witness_bad(sized):
    c, key, pool = sized, sized["key"], sized["pool"]
    cap = key.fuse()
    assert cap >= 2 and cap <= POOL
    before = key.h_form()["retries"]
    wits, rs, ss, want = pool.batch(cap, bad=(cap - 1,))
    got = _prove_device(key, wits, rs, ss)
    assert got == want and len(set(got)) == cap
    assert key.h_form()["retries"] == before + 1


def test_full_groups_reach_the_last_counter_word(sized):
    """Two groups of key.fuse() witnesses each (the only way a batch call fills a group): the last witness of the second group is
    bad, so the slot's last counter word is the one that says so."""
    c, key, pool = sized, sized["key"], sized["pool"]
    cap = key.fuse()
    assert cap >= 2 and 2 * cap <= POOL
    before = key.h_form()["retries"]
    wits, rs, ss, want = pool.batch(2 * cap, bad=(2 * cap - 1,))
    key.prof_enable(True)
    try:
        key.prof_reset()
        got = _prove_device(key, wits, rs, ss)
        spmv = key.prof()["spmv_a"][1]
    finally:
        key.prof_enable(False)
        key.prof_reset()
    assert got == want and len(set(got)) == 2 * cap
    assert key.h_form()["retries"] == before + 1
    assert spmv == 3  # two groups and ONE of them again


def test_bad_witness_in_the_second_group(sized):
    """key.fuse() + 3 witnesses are two groups, one per slot, both in flight; the bad witness is in the second, and only that group
    is proved again: three calcH runs in all."""
    c, key, pool = sized, sized["key"], sized["pool"]
    cap = key.fuse()
    assert cap >= 2 and cap + 3 <= POOL
    n = cap + 3
    first = (n + 1) // 2  # witnesses of the first group (group_count: sizes that differ by at most one, the larger first)
    bad = first + 2
    assert first < bad < n
    before = key.h_form()["retries"]
    wits, rs, ss, want = pool.batch(n, bad=(bad,))
    key.prof_enable(True)
    try:
        key.prof_reset()
        got = _prove_device(key, wits, rs, ss)
        spmv = key.prof()["spmv_a"][1]
    finally:
        key.prof_enable(False)
        key.prof_reset()
    assert got == want and len(set(got)) == n
    assert key.h_form()["retries"] == before + 1
    assert spmv == 3  # the first group was not proved again


# ---------------------------------------------------------------- 4. host buffers
def test_bad_witness_inside_a_group_from_host_buffers(sized):
    c, key, pool = sized, sized["key"], sized["pool"]
    assert key.fuse() >= 2
    before = key.h_form()["retries"]
    wits, rs, ss, want = pool.batch(5, bad=(2,))
    got = key.prove_batch(wits, rs, ss)
    assert got == want and len(set(got)) == 5
    assert key.h_form()["retries"] == before + 1


# ---------------------------------------------------------------- 5. wide C rows under a batch
def _wide_c_rows():
    """Domain 2^7, three public signals.  Every third constraint carries a public signal on its C side; constraint 40 has 9 terms on
    its C side (one more than spmv_kernel keeps: SPMV_WIDE = 8) and constraint 100 has 70 (more than the 64 lanes that share a row in
    spmv_wide_kernel, so one lane takes two terms), public signals among them."""
    rnd = random.Random(0x5A4B0500)
    p, m = 3, 128
    w = [1] + [rnd.randrange(1, R) for _ in range(p)]
    rows = []
    for row in range(m - p - 1):
        n = len(w)
        A = sorted({n - 1: 1, rnd.randrange(n): rnd.randrange(1, R)}.items())
        B = [(rnd.randrange(n), rnd.randrange(1, R))]
        val = sum(cf * w[s] for s, cf in A) * sum(cf * w[s] for s, cf in B) % R
        C = []
        extra = {40: 8, 100: 69}.get(row, 0)
        if extra:
            C = [(s, rnd.randrange(1, R)) for s in sorted(rnd.sample(range(p + 1, n), extra - p) + [1, 2, 3])]
        elif row % 3 == 0:
            C = [(1 + rnd.randrange(p), rnd.randrange(1, R))]
        val = (val - sum(cf * w[s] for s, cf in C)) % R
        rows.append((A, B, C + [(n, 1)]))
        w.append(val)
    circ = dict(nVars=len(w), nPublic=p, nConstraints=len(rows), domainSize=m, rows=rows, witness=w)
    assert g.check_r1cs(circ)
    assert sorted(len(C) for _, _, C in rows)[-2:] == [9, 70]
    return circ


def test_wide_c_rows_in_a_fused_group():
    import zkr_hip
    c = _setup(_wide_c_rows())
    key = c["key"]
    try:
        assert key.fuse() >= 2
        assert key.h_form() == {"form": EVAL, "retries": 0}
        rs, ss = [77, 78, 79], [99, 98, 97]
        got = _prove_device(key, [c["wb"]] * 3, rs, ss)
        assert got == [_closed(c, r, s) for r, s in zip(rs, ss)] == [coracle.prove(c["pkb"], c["wb"], r, s) for r, s in zip(rs, ss)]
        assert key.h_form() == {"form": EVAL, "retries": 0}
        assert all(zkr_hip.verify(c["vk"], proof, c["w"][1:4]) for proof in got)
    finally:
        key.close()


# ---------------------------------------------------------------- 6. C and H reduced by separate chains
def test_c_and_h_reduced_apart_in_a_fused_group():
    """100 signals under a domain of 2^8 (tests/layout_cases.py): C' and E' are reduced by a chain each, with three proofs' bucket
    sets end to end in both."""
    from layout_cases import few_signals_many_constraints
    lc = few_signals_many_constraints()
    c = _setup(lc["circ"])
    key = c["key"]
    try:
        win = key.windows()
        assert key.fuse() >= 2
        assert key.h_form() == {"form": EVAL, "retries": 0} and win["C"][0] != win["H"][0]
        wits = [c["wb"], _bad_witness(lc["circ"]["nVars"], 8), c["wb"]]
        rs, ss = [5, 6, 7], [7, 8, 9]
        got = _prove_device(key, wits, rs, ss)
        assert got == [coracle.prove(lc["pkb"], wb, r, s) for wb, r, s in zip(wits, rs, ss)]  # the oracle on the ORACLE's setup of the circuit
        assert len(set(got)) == 3 and key.h_form()["retries"] == 1
    finally:
        key.close()


# ---------------------------------------------------------------- 7. derived tables
def test_derived_tables_in_a_fused_group(sized):
    """A key loaded from websnark bytes, its side tables derived from its own points (zkr_key_eval_tables)."""
    import zkr_hip
    c, twin, pool = sized, sized["key"], sized["pool"]
    key = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    try:
        assert key.fuse() >= 2
        assert key.eval_tables(c["r1cs"]) is True and key.h_form() == {"form": EVAL, "retries": 0}
        wits, rs, ss, want = pool.batch(4)
        got = _prove_device(key, wits, rs, ss)
        assert got == _prove_device(twin, wits, rs, ss) == want
        assert key.h_form() == {"form": EVAL, "retries": 0}
    finally:
        key.close()
