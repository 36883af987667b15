"""GPU: ONE proof over several shards with H in evaluation form (include/zkr.h zkr_key_shard_opts, zkr_prove_sharded_last_h_form;
csrc/zkr_prove.hip calc_h_eval / calc_h_split, csrc/zkr_multi.hip run_sharded) is the bytes of every other route.

Keys come from zkr_setup_r1cs with injected toxic scalars, as in tests/test_gpu_eval_h.py: closed form from the toxic scalars, the
C oracle on the websnark rendering of the same setup, the verifier.  Shards sit side by side on device i % device_count(): on a
one-GPU box the cross passes are plain loads and stores, the schedule, the barriers and the side tables are the node's."""
import random
import re

import pytest

import coracle
import groth16 as g
from groth16 import R

pytestmark = pytest.mark.gpu

TOX = ("t", "alfa", "beta", "gamma", "delta")
RS = (0x1234567890ABCDEF, 0x0FEDCBA987654321)
# (log_m, parts): replicated with fewer than 64 columns per cross pass and shards that own no C point; split with two passes per
# block transform; split at exactly 64 columns; replicated over ranges that are no aligned blocks; split over four
CASES = [(7, 8), (12, 2), (12, 8), (12, 3), (14, 4)]
SPLIT = {(12, 2), (12, 8), (14, 4)}

_setups, _shards = {}, {}


def _r1cs(circ):
    import zkr_hip
    return zkr_hip.binarify_r1cs(dict(nVars=circ["nVars"], nPublic=circ["nPublic"], constraints=[[list(lc) for lc in row] for row in circ["rows"]]))


def _setup(circ):
    """The key (with side tables), its verifying key, the same setup as websnark bytes, and the references of the circuit's own
    witness under RS -- computed once and read by every test."""
    import zkr_hip
    tox = g.toxic_from_seed(0x5A4B00FF)
    r1cs = _r1cs(circ)
    toxic = [tox[k] for k in TOX]
    key, vk = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=toxic)
    pkb, _ = zkr_hip.setup_r1cs_websnark(r1cs, toxic=toxic)
    wb = g.binarify_witness(circ["witness"])
    want = g.proof_bytes(g.proof_from_toxic(circ, tox, circ["witness"], *RS))
    assert want == coracle.prove(pkb, wb, *RS)
    assert key.h_form()["form"] == "evaluation"
    return dict(circ=circ, tox=tox, key=key, vk=vk, pkb=pkb, r1cs=r1cs, wb=wb, want=want)


def _sized(log_m):
    if log_m not in _setups:
        c = _setup(g.synth_circuit(1 << log_m, 7, 0x5A4B0001))
        c["log_m"] = log_m
        _setups[log_m] = c
    return _setups[log_m]


def _cut(key, parts, side_tables=True):
    import zkr_hip
    nd = zkr_hip.device_count()
    return [key.shard(i, parts, device=i % nd, side_tables=side_tables) for i in range(parts)]


def _case(log_m, parts):
    """(setup, shards with side tables) of a case; the shards of a case are shared, so their `retries` only ever grow."""
    c = _sized(log_m)
    if (log_m, parts) not in _shards:
        _shards[(log_m, parts)] = _cut(c["key"], parts)
    return c, _shards[(log_m, parts)]


@pytest.fixture(scope="module", autouse=True)
def _keys_go_with_the_module():
    yield
    for shards in _shards.values():
        for sh in shards:
            sh.close()
    for c in _setups.values():
        c["key"].close()
    _shards.clear()
    _setups.clear()


def _on_devices(wb, shards):
    import torch
    ts = [torch.frombuffer(bytearray(wb), dtype=torch.uint8).to("cuda:%d" % sh.device) for sh in shards]
    torch.cuda.synchronize()
    return ts


def _retries(shards):
    return [sh.h_form()["retries"] for sh in shards]


def _unsatisfied_rows(circ, w):
    return sum(1 for A, B, C in circ["rows"]
               if sum(cf * w[s] for s, cf in A) * sum(cf * w[s] for s, cf in B) % R != sum(cf * w[s] for s, cf in C) % R)


@pytest.mark.parametrize("log_m,parts", CASES)
def test_sharded_proof_equals_the_references(log_m, parts, monkeypatch):
    import zkr_hip
    c, shards = _case(log_m, parts)
    key, wb, want = c["key"], c["wb"], c["want"]
    assert all(sh.h_form()["form"] == "evaluation" for sh in shards)
    before = _retries(shards)
    assert key.prove(wb, *RS) == want
    assert zkr_hip.prove_sharded(shards, wb, *RS) == want
    hf = zkr_hip.sharded_last_h_form()
    assert hf == {"form": "evaluation", "reason": "every shard has side tables"}
    split = (log_m, parts) in SPLIT
    assert zkr_hip.sharded_last_form()["form"] == ("split" if split else "replicated")
    stats = zkr_hip.sharded_split_stats()
    assert (stats is not None and len(stats) == parts and all(ms > 0 for row in stats for ms in row[:4])) if split else stats is None
    dev = _on_devices(wb, shards)
    for _ in range(3):  # the barriers, the in-place cross passes and the counters survive being used again
        assert zkr_hip.prove_sharded_device(shards, [t.data_ptr() for t in dev], *RS) == want
        assert zkr_hip.sharded_last_h_form()["form"] == "evaluation"
    wb2 = zkr_hip.synth_witness(log_m, 7, 0x5A4B0001, 4100 + parts)
    assert zkr_hip.prove_sharded(shards, wb2, 5, 6) == coracle.prove(c["pkb"], wb2, 5, 6) == key.prove(wb2, 5, 6)
    assert zkr_hip.sharded_last_h_form()["form"] == "evaluation" and _retries(shards) == before
    # a shard on its own keeps the coefficient form: its records combine to the same proof
    assert key.prove_combine([sh.prove_partial(wb) for sh in shards], *RS) == want
    assert _retries(shards) == before
    # the first-use check of a fresh set compares split against replicated in the evaluation form
    monkeypatch.setenv("ZKR_SHARD_SPLIT_CHECK", "1")
    fresh = _cut(key, parts)
    assert zkr_hip.prove_sharded(fresh, wb, *RS) == want
    assert zkr_hip.sharded_last_h_form()["form"] == "evaluation"
    form = zkr_hip.sharded_last_form()
    assert (form["form"] == "split" and "proved both ways" in form["reason"]) if split else form["form"] == "replicated"
    assert zkr_hip.prove_sharded(fresh, wb, *RS) == want and "both ways" not in zkr_hip.sharded_last_form()["reason"]
    assert _retries(fresh) == [0] * parts
    for sh in fresh:
        sh.close()


@pytest.mark.parametrize("log_m,parts", [(12, 2), (14, 4)])
def test_fewer_transform_launches_per_shard(log_m, parts):
    """The stage timers of a shard: the split calcH in evaluation form launches strictly fewer transform passes than the coefficient
    form on a shard set cut without tables (two cross passes instead of three in phase 2, no S' on the block, no cross inverse
    transform nor block transform of D'); the product stands where the combination stood, one launch either way."""
    import zkr_hip
    c, shards = _case(log_m, parts)
    plain = _cut(c["key"], parts, side_tables=False)
    counts = {}
    for tag, group in (("evaluation", shards), ("coefficients", plain)):
        assert zkr_hip.prove_sharded(group, c["wb"], *RS) == c["want"]  # warm, and the form is what the tag says
        assert zkr_hip.sharded_last_h_form()["form"] == tag and zkr_hip.sharded_last_form()["form"] == "split"
        for sh in group:
            sh.prof_enable(True)
            sh.prof_reset()
        assert zkr_hip.prove_sharded(group, c["wb"], *RS) == c["want"]
        counts[tag] = [(sh.prof()["ntt_pass"][1], sh.prof()["combine_h"][1]) for sh in group]
        for sh in group:
            sh.prof_enable(False)
    print("ntt_pass / combine_h launches per shard at 2^%d x %d:" % (log_m, parts), counts)
    for (ne, ce), (nc, cc) in zip(counts["evaluation"], counts["coefficients"]):
        assert 0 < ne < nc and ce == cc == 1
    for sh in plain:
        sh.close()


@pytest.mark.parametrize("log_m,parts", [(12, 2), (12, 3)])
def test_unsatisfying_witness_goes_again_on_every_shard(log_m, parts):
    import zkr_hip
    c, shards = _case(log_m, parts)
    circ, w = c["circ"], c["circ"]["witness"]
    rnd = random.Random(97 * parts)
    last = list(w)
    last[-1] = (last[-1] + 1) % R  # only the LAST block of the domain sees a bad row: the test of the sum over the shards
    n_last = _unsatisfied_rows(circ, last)
    assert 0 < n_last < 8 and all(r >= (parts - 1) * (1 << log_m) // parts for r, (A, B, C) in enumerate(circ["rows"])
                                  if sum(cf * last[s] for s, cf in A) * sum(cf * last[s] for s, cf in B) % R != sum(cf * last[s] for s, cf in C) % R)
    anything = [1] + [rnd.randrange(R) for _ in range(len(w) - 1)]
    for bad in (anything, last):
        bad_wb = g.binarify_witness(bad)
        before = _retries(shards)
        r, s = rnd.randrange(R), rnd.randrange(R)
        assert zkr_hip.prove_sharded(shards, bad_wb, r, s) == coracle.prove(c["pkb"], bad_wb, r, s)
        hf = zkr_hip.sharded_last_h_form()
        assert hf["form"] == "coefficients"
        m = re.fullmatch(r"witness left (\d+) rows unsatisfied: proved again through the coefficient form", hf["reason"])
        assert m and int(m.group(1)) == _unsatisfied_rows(circ, bad)
        assert _retries(shards) == [b + 1 for b in before]
        dev = _on_devices(bad_wb, shards)
        assert zkr_hip.prove_sharded_device(shards, [t.data_ptr() for t in dev], r, s) == coracle.prove(c["pkb"], bad_wb, r, s)
        assert _retries(shards) == [b + 2 for b in before]
        # the next good witness: evaluation form again, proved once
        assert zkr_hip.prove_sharded(shards, c["wb"], *RS) == c["want"]
        assert zkr_hip.sharded_last_h_form()["form"] == "evaluation" and _retries(shards) == [b + 2 for b in before]


def test_tables_derived_from_the_points_cut_to_the_same_bytes():
    """load_websnark + eval_tables(r1cs) + shard(side_tables=True) against the shards of the setup's own key."""
    import zkr_hip
    c, shards = _case(12, 2)
    loaded = zkr_hip.ProvingKey.load_websnark(c["pkb"])
    assert loaded.eval_tables(c["r1cs"]) and loaded.h_form()["form"] == "evaluation"
    cut = _cut(loaded, 2)
    assert all(sh.h_form()["form"] == "evaluation" for sh in cut)
    assert all(a.eval_tables_equal(b) for a, b in zip(cut, shards))
    assert not cut[0].eval_tables_equal(shards[1]) and not cut[0].eval_tables_equal(loaded)  # another part; a shard and a whole key
    assert zkr_hip.prove_sharded(cut, c["wb"], *RS) == c["want"] and zkr_hip.sharded_last_h_form()["form"] == "evaluation"
    with pytest.raises(zkr_hip.ZkrError, match="shard"):
        cut[0].eval_tables(c["r1cs"])  # derive on the whole key, then cut
    for sh in cut:
        sh.close()
    loaded.close()


def test_public_signal_in_c_cut_in_two():
    """2^7 with C' points on public signals (tests/test_gpu_eval_h.py _public_in_c): the shard of the witness' head owns them."""
    import zkr_hip
    from test_gpu_eval_h import _public_in_c
    c = _setup(_public_in_c())
    cut = _cut(c["key"], 2)
    assert all(sh.h_form()["form"] == "evaluation" for sh in cut)
    proof = zkr_hip.prove_sharded(cut, c["wb"], *RS)
    assert proof == c["want"] and zkr_hip.verify(c["vk"], proof, c["circ"]["witness"][1:4])
    assert zkr_hip.sharded_last_h_form()["form"] == "evaluation" and _retries(cut) == [0, 0]
    for sh in cut:
        sh.close()
    c["key"].close()


def test_levels_copied_when_the_window_stays(monkeypatch):
    """ZKR_MSM_C=8 while the key and the shards are built: the shards keep the whole key's window, so every level of C' and E' is
    copied, not rebuilt.  Shards of the same key cut without the knob choose their own window and rebuild from level 0: other
    bytes (other levels), the same proofs."""
    import zkr_hip
    monkeypatch.setenv("ZKR_MSM_C", "8")
    c = _setup(g.synth_circuit(1 << 12, 7, 0x5A4B0001))
    key = c["key"]
    copied = _cut(key, 2)
    monkeypatch.delenv("ZKR_MSM_C")
    rebuilt = _cut(key, 2)
    assert all(sh.windows()["H"][0] == 8 == key.windows()["H"][0] and sh.windows()["C"][0] == 8 for sh in copied)
    assert all(sh.windows()["H"][0] != 8 for sh in rebuilt)
    for group in (copied, rebuilt):
        assert all(sh.h_form()["form"] == "evaluation" for sh in group)
        assert zkr_hip.prove_sharded(group, c["wb"], *RS) == c["want"]
        assert zkr_hip.sharded_last_h_form()["form"] == "evaluation" and zkr_hip.sharded_last_form()["form"] == "split"
    assert not any(a.eval_tables_equal(b) for a, b in zip(copied, rebuilt))
    for sh in copied + rebuilt:
        sh.close()
    key.close()


def test_fall_backs_to_the_coefficient_form(monkeypatch):
    import zkr_hip
    c, shards = _case(12, 2)
    key, wb, want = c["key"], c["wb"], c["want"]
    # a whole key without tables: the flag gives a coefficient-form shard and says why
    bare, _ = zkr_hip.ProvingKey.setup_r1cs(c["r1cs"], toxic=[c["tox"][k] for k in TOX], side_tables=False)
    plain = _cut(bare, 2)
    assert "no side tables" in zkr_hip.lib().zkr_last_error().decode()
    assert all(sh.h_form() == {"form": "coefficients", "retries": 0} for sh in plain)
    assert zkr_hip.prove_sharded(plain, wb, *RS) == want
    assert zkr_hip.sharded_last_h_form() == {"form": "coefficients", "reason": "shard 0 has no side tables"}
    # one shard of the set cut without tables
    mixed = [shards[0], key.shard(1, 2, device=shards[1].device)]
    assert zkr_hip.prove_sharded(mixed, wb, *RS) == want
    assert zkr_hip.sharded_last_h_form() == {"form": "coefficients", "reason": "shard 1 has no side tables"}
    # ... or its tables dropped
    own = _cut(key, 2)
    assert zkr_hip.prove_sharded(own, wb, *RS) == want and zkr_hip.sharded_last_h_form()["form"] == "evaluation"
    own[1].drop_eval_tables()
    assert own[1].h_form()["form"] == "coefficients"
    assert zkr_hip.prove_sharded(own, wb, *RS) == want
    assert zkr_hip.sharded_last_h_form() == {"form": "coefficients", "reason": "shard 1 has no side tables"}
    # the knob: shards that have tables prove through the coefficient form; shards cut under it get none
    monkeypatch.setenv("ZKR_H_FORM", "coefficients")
    assert zkr_hip.prove_sharded(shards, wb, *RS) == want
    assert zkr_hip.sharded_last_h_form() == {"form": "coefficients", "reason": "ZKR_H_FORM=coefficients"}
    under = _cut(key, 2)
    assert "ZKR_H_FORM=coefficients" in zkr_hip.lib().zkr_last_error().decode()
    assert all(sh.h_form()["form"] == "coefficients" for sh in under)
    monkeypatch.delenv("ZKR_H_FORM")
    assert zkr_hip.prove_sharded(under, wb, *RS) == want and zkr_hip.sharded_last_h_form()["reason"] == "shard 0 has no side tables"
    assert zkr_hip.prove_sharded(shards, wb, *RS) == want and zkr_hip.sharded_last_h_form()["form"] == "evaluation"
    with pytest.raises(zkr_hip.ZkrError, match="shard"):
        shards[0].eval_tables(c["r1cs"])
    for sh in plain + mixed[1:] + own + under:
        sh.close()
    bare.close()
