"""CPU: MiMC7, ecdh and the cipher of crypto.ts:86-141 as host calls (csrc/zkr_crypto.hip over csrc/crypto_program.hpp) against
published values (tests/golden/mimc7_kat.json), against an independent model (tests/crypto_model.py) and against their own
refusals, which come before any device is looked at."""
import functools
import json
import os
import random

import pytest

import crypto_model as m
import rollup as o
import wallet_cases as wc
import zkr_hip
from zkr_hip import rollup as n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = o.R
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "mimc7_kat.json")))
OFF_CURVE = (1, 1)   # 168700 + 1 != 1 + 168696


def _refused(call, *words):
    with pytest.raises(zkr_hip.ZkrError) as e:
        call()
    assert e.value.code == -5, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@functools.lru_cache(maxsize=None)
def edge_messages(arity):
    """One message per key of the wallet list: its random message with elements replaced in turn by 0, 1 and r - 1."""
    rng = random.Random(0x5A4B0300 + arity)
    out = []
    for t, msg in enumerate(wc.messages(arity)):
        msg = [int(v) for v in msg]
        if t % 4:
            msg[rng.randrange(arity)] = (0, 1, R - 1)[t % 4 - 1]
        if t == 4:
            msg = [R - 1] * arity
        out.append(tuple(msg))
    return tuple(out)


def _check_kat(constants, hash_, multi_hash):
    for i, v in KAT["constants"].items():
        assert constants[int(i)] == int(v), i
    assert len(constants) == 91 and constants[0] == 0
    assert hash_(1, 2) == int(KAT["hash_1_2"])
    for e in KAT["multihash"]:
        assert multi_hash([int(x) for x in e["in"]]) == int(e["out"], 16), e["in"]


def test_model_reproduces_the_published_values():
    _check_kat(m.constants(), m.mimc7_hash, m.multi_hash)


def test_host_calls_reproduce_the_published_values_and_the_model_constants():
    _check_kat(n.mimc7_round_constants(), n.mimc7_hash, n.mimc7_multi_hash)
    assert tuple(n.mimc7_round_constants()) == m.constants()
    rng = random.Random(0x5A4B0301)
    for x, k in [(0, 0), (R - 1, R - 1), (0, R - 1)] + [(rng.randrange(R), rng.randrange(R)) for _ in range(8)]:
        assert n.mimc7_hash(x, k) == m.mimc7_hash(x, k), (x, k)
        assert n.mimc7_multi_hash([x, k, 1], key=k) == m.multi_hash([x, k, 1], k)
    assert n.mimc7_multi_hash([], key=7) == 7


def test_ecdh_is_symmetric_on_the_reference_key_pairs():
    (a, pa), (b, pb) = wc.kat_pairs()
    want = int(KAT["ecdh_reference_pairs"])
    assert m.ecdh(a, pb) == m.ecdh(b, pa) == want   # crypto.test.ts:22-27
    assert n.ecdh(a, pb) == n.ecdh(b, pa) == want


def test_ecdh_equals_the_model_on_the_key_list_and_on_special_points():
    keys, pubs = wc.keys(), wc.oracle_pubs()
    for t, (k, want) in enumerate(zip(keys, m.list_shared_keys())):
        assert n.ecdh(k, pubs[(t + 1) % len(keys)]) == want, k
    for pub in ((0, 1), (0, R - 1)):   # the identity and the point of order two: accepted, as in the reference
        assert o.bj_on_curve(pub) and n.ecdh(keys[3], pub) == m.ecdh(keys[3], pub) == 0


@pytest.mark.parametrize("arity", [1, 5, 8])
def test_cipher_equals_the_model_and_round_trips(arity):
    for k, msg in zip(wc.keys(), edge_messages(arity)):
        enc = n.encrypt(msg, k)
        assert enc == m.encrypt(list(msg), k), (k, arity)
        assert all(e < 2 * R for e in enc["msg"])
        assert n.decrypt(enc, k) == list(msg) == m.decrypt(enc, k)
        reduced = {"iv": enc["iv"], "msg": [e % R for e in enc["msg"]]}   # a ciphertext reduced mod r opens to the same message
        assert n.decrypt(reduced, k) == list(msg)


def test_integer_sum_is_kept_where_it_passes_r():
    seen = 0
    for k, msg in zip(wc.keys(), edge_messages(5)):
        seen += sum(e >= R for e in n.encrypt(msg, k)["msg"])
    assert seen > 0   # the case list does reach sums past r, so the comparison above covers them


def test_ecdh_compositions():
    (a, pa), (b, pb) = wc.kat_pairs()
    msg = [3, 0, R - 1, 12345]
    enc = n.ecdh_encrypt(msg, a, pb)
    assert enc == m.encrypt(msg, m.ecdh(a, pb))
    assert n.ecdh_decrypt(enc, b, pa) == msg


def test_iv_of_r_minus_one_wraps_the_counter():
    k = wc.keys()[5]
    enc = {"iv": R - 1, "msg": [5, R + 7, 2 * R - 1]}
    want = m.decrypt(enc, k)
    assert want[1] == (7 - m.mimc7_hash(k, 0)) % R   # element 1 is under counter 0
    assert n.decrypt(enc, k) == want


def test_refusals_name_item_and_element():
    (a, pa), _ = wc.kat_pairs()
    _refused(lambda: n.mimc7_hash(R, 0), "x >= r")
    _refused(lambda: n.mimc7_hash(0, R), "key >= r")
    _refused(lambda: n.mimc7_multi_hash([1, R], 0), "element 1")
    _refused(lambda: n.mimc7_multi_hash([1], R), "key >= r")
    _refused(lambda: n.ecdh(R, pa), "item 0", "private key >= r")
    _refused(lambda: n.ecdh(a, (R, pa[1])), "item 0", "coordinate 0")
    _refused(lambda: n.ecdh(a, (pa[0], R)), "item 0", "coordinate 1")
    _refused(lambda: n.ecdh(a, OFF_CURVE), "item 0", "not on the curve")
    _refused(lambda: n.encrypt([1, 2], R), "item 0", "key >= r")
    _refused(lambda: n.encrypt([1, 2, R], 3), "item 0", "message element 2")
    _refused(lambda: n.encrypt([], 3), "arity")
    _refused(lambda: n.decrypt({"iv": R, "msg": [1]}, 3), "item 0", "iv >= r")
    _refused(lambda: n.decrypt({"iv": 1, "msg": [1, 2 * R]}, 3), "item 0", "ciphertext element 1", "2r")
    _refused(lambda: n.decrypt({"iv": 1, "msg": [1]}, R), "item 0", "key >= r")
    _refused(lambda: n.encrypt([1, 1 << 256], 3))
    assert n.decrypt({"iv": 1, "msg": [2 * R - 1]}, 3) == m.decrypt({"iv": 1, "msg": [2 * R - 1]}, 3)


def test_batch_refusals_come_before_any_device_is_looked_at():
    """Every argument check of the batch calls answers on a machine without a GPU, naming the first offending item; device 99
    does not exist anywhere."""
    keys, pubs = list(wc.keys()[:6]), list(wc.oracle_pubs()[:6])
    msgs = [list(x) for x in edge_messages(5)[:6]]
    encs = [{"iv": 1, "msg": list(x)} for x in msgs]
    bad = lambda xs, t, v: xs[:t] + [v] + xs[t + 1:]
    _refused(lambda: n.ecdh_batch(bad(keys, 4, R), pubs, device=99), "item 4", "private key")
    _refused(lambda: n.ecdh_batch(keys, bad(pubs, 2, OFF_CURVE), device=99), "item 2", "not on the curve")
    _refused(lambda: n.ecdh_batch(keys, bad(pubs, 3, (R, 1)), device=99), "item 3", "coordinate 0")
    _refused(lambda: n.ecdh_batch(keys, pubs[:5], device=99))
    _refused(lambda: n.encrypt_batch(bad(keys, 5, R), msgs, device=99), "item 5", "key >= r")
    _refused(lambda: n.encrypt_batch(keys, bad(msgs, 3, [1, 2, 3, R, 5]), device=99), "item 3", "message element 3")
    _refused(lambda: n.encrypt_batch(keys, bad(msgs, 3, [1, 2, 3]), device=99), "item 3")   # ragged
    _refused(lambda: n.encrypt_batch(keys, [[]] * 6, device=99), "arity")
    _refused(lambda: n.decrypt_batch(keys, bad(encs, 1, {"iv": R, "msg": msgs[1]}), device=99), "item 1", "iv >= r")
    _refused(lambda: n.decrypt_batch(keys, bad(encs, 2, {"iv": 0, "msg": [0, 2 * R, 0, 0, 0]}), device=99), "item 2", "ciphertext element 1")
    _refused(lambda: n.ecdh_encrypt_batch(keys, bad(pubs, 0, OFF_CURVE), msgs, device=99), "item 0", "not on the curve")
    _refused(lambda: n.ecdh_encrypt_batch(keys, pubs, bad(msgs, 5, [R] * 5), device=99), "item 5", "message element 0")
    _refused(lambda: n.ecdh_decrypt_batch(bad(keys, 1, R), pubs, encs, device=99), "item 1", "private key")
    _refused(lambda: n.ecdh_decrypt_batch(keys, pubs, bad(encs, 4, {"iv": 2, "msg": [1, 2]}), device=99), "item 4")
    # in order: a well-formed call gets as far as the device, and no further
    with pytest.raises(zkr_hip.ZkrError) as e:
        n.ecdh_encrypt_batch(keys, pubs, msgs, device=99)
    assert e.value.code == -1 and "no CPU fallback" in str(e.value)
    for call in (lambda: n.ecdh_batch([], []), lambda: n.encrypt_batch([], []), lambda: n.decrypt_batch([], []),
                 lambda: n.ecdh_encrypt_batch([], [], []), lambda: n.ecdh_decrypt_batch([], [], [])):
        assert call() == []


def test_null_arguments_and_empty_lists_at_the_c_abi():
    L = zkr_hip.lib()
    buf = bytes(64 * 4)
    assert L.zkr_mimc7_round_constants(None) == -5 and L.zkr_mimc7_hash(None, buf, None) == -5
    assert L.zkr_babyjub_ecdh(None, buf, None) == -5 and L.zkr_mimc7_encrypt(buf, None, 1, None, None) == -5
    assert L.zkr_mimc7_decrypt(buf, buf, None, 1, None) == -5
    assert L.zkr_babyjub_ecdh_batch(None, buf, 2, None, 0) == -5 and L.zkr_mimc7_encrypt_batch(buf, None, 1, 2, None, None, 0) == -5
    assert L.zkr_mimc7_decrypt_batch(buf, buf, None, 1, 2, None, 0) == -5
    assert L.zkr_ecdh_encrypt_batch(buf, None, buf, 1, 2, None, None, 0) == -5
    assert L.zkr_ecdh_decrypt_batch(buf, buf, None, buf, 1, 2, None, 0) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_babyjub_ecdh_batch(None, None, 0, None, 0) == 0 and L.zkr_mimc7_encrypt_batch(None, None, 5, 0, None, None, 0) == 0
    assert L.zkr_mimc7_decrypt_batch(None, None, None, 5, 0, None, 0) == 0 and L.zkr_ecdh_encrypt_batch(None, None, None, 5, 0, None, None, 0) == 0
    assert L.zkr_ecdh_decrypt_batch(None, None, None, None, 5, 0, None, 0) == 0
    for arity in (0, 65537):
        assert L.zkr_mimc7_encrypt_batch(buf, buf, arity, 1, buf, buf, 0) == -5 and b"arity" in L.zkr_last_error()
