"""GPU: ecdh and the MiMC7 cipher in bulk (csrc/zkr_crypto.hip) against the host calls they stand in for, item by item and bit for
bit, at the sizes where these kernels can go wrong: one item, one short of a wavefront, a wavefront, one more, and 70; for the
keystream kernel, whose grid is the flat n x arity list of elements, shapes where that grid ends inside a wavefront while no
message does ((13, 5): 65 elements) and where one message spans a whole wavefront ((3, 64))."""
import random

import pytest

import crypto_model as m
import wallet_cases as wc
import zkr_hip
from zkr_hip import rollup as n

pytestmark = pytest.mark.gpu
R = n.SNARK_FIELD_SIZE
SIZES = (1, 63, 64, 65, 70)
SHAPES = ((1, 1), (13, 5), (70, 5), (3, 64), (64, 1))


def _messages(count, arity):
    """`count` messages of `arity` elements from {0, 1, r - 1, random}."""
    rng = random.Random(0x5A4B0400 + 1000 * count + arity)
    return [[rng.choice((0, 1, R - 1, rng.randrange(R), rng.randrange(R))) for _ in range(arity)] for _ in range(count)]


@pytest.fixture(scope="module")
def host():
    """What the host calls give for the case list, computed once: key t meets the public key of key t + 1."""
    keys = list(wc.keys())
    pubs = [n.gen_public_key(k) for k in keys]
    peers = pubs[1:] + pubs[:1]
    return {"keys": keys, "pubs": pubs, "peers": peers, "shared": [n.ecdh(k, p) for k, p in zip(keys, peers)]}


@pytest.fixture(scope="module")
def cipher_cases(host):
    """(n, arity) -> (keys, messages, what `encrypt` gives for each), computed once on the host."""
    out = {}
    for count, arity in SHAPES:
        keys, msgs = host["shared"][:count], _messages(count, arity)
        out[count, arity] = (keys, msgs, [n.encrypt(x, k) for x, k in zip(msgs, keys)])
    return out


@pytest.mark.parametrize("count", SIZES)
def test_ecdh_batch_equals_the_host_call(host, count):
    assert len(host["keys"]) == 70
    at = 0 if count == 70 else 3   # from the first reference key on
    got = n.ecdh_batch(host["keys"][at:at + count], host["peers"][at:at + count])
    assert got == host["shared"][at:at + count]


def test_ecdh_batch_equals_the_model_and_takes_special_points(host):
    keys = host["keys"][:6]
    pubs = [(0, 1), (0, R - 1)] + host["peers"][2:6]   # the identity and the point of order two
    got = n.ecdh_batch(keys, pubs)
    assert got == [m.ecdh(k, p) for k, p in zip(keys, pubs)] and got[:2] == [0, 0]


@pytest.mark.parametrize("count,arity", SHAPES)
def test_cipher_batches_equal_the_host_calls(cipher_cases, count, arity):
    keys, msgs, want = cipher_cases[count, arity]
    got = n.encrypt_batch(keys, msgs)
    assert got == want
    assert n.decrypt_batch(keys, got) == msgs
    reduced = [{"iv": e["iv"], "msg": [v % R for v in e["msg"]]} for e in got]
    assert n.decrypt_batch(keys, reduced) == msgs
    if (count, arity) == (13, 5):
        assert got[0] == m.encrypt(msgs[0], keys[0]) and any(v >= R for e in got for v in e["msg"])


@pytest.mark.parametrize("count", SIZES)
def test_cipher_batches_at_every_size(host, count):
    keys, msgs = host["shared"][:count], _messages(count, 2)
    want = [n.encrypt(x, k) for x, k in zip(msgs, keys)]
    assert n.encrypt_batch(keys, msgs) == want
    assert n.decrypt_batch(keys, want) == [n.decrypt(e, k) for e, k in zip(want, keys)] == msgs
    assert n.ecdh_encrypt_batch(host["keys"][:count], host["peers"][:count], msgs) == want
    assert n.ecdh_decrypt_batch(host["keys"][:count], host["peers"][:count], want) == msgs


def test_ecdh_encrypt_then_decrypt_with_the_parties_swapped(host):
    keys, pubs = host["keys"], host["pubs"]
    for count, arity in ((70, 5), (1, 1), (3, 64)):
        a, b = keys[:count], (keys[1:] + keys[:1])[:count]
        pa, pb = pubs[:count], host["peers"][:count]
        msgs = _messages(count, arity)
        encs = n.ecdh_encrypt_batch(a, pb, msgs)
        assert encs == n.encrypt_batch(n.ecdh_batch(a, pb), msgs)
        assert encs[0] == n.ecdh_encrypt(msgs[0], a[0], pb[0])
        assert n.ecdh_decrypt_batch(b, pa, encs) == msgs


def test_iv_of_r_minus_one_at_arity_three(host):
    keys = host["shared"][:5]
    encs = [{"iv": R - 1, "msg": [5 + t, R + 7, 2 * R - 1]} for t in range(5)]
    want = [n.decrypt(e, k) for e, k in zip(encs, keys)]
    assert want[0] == m.decrypt(encs[0], keys[0])
    assert n.decrypt_batch(keys, encs) == want


def test_refusals_come_before_a_launch_and_an_empty_list_works(host):
    keys, peers = host["keys"][:4], host["peers"][:4]
    msgs = _messages(4, 3)
    for call, words in ((lambda: n.ecdh_batch(keys[:3] + [R], peers), ("item 3", "private key")),
                        (lambda: n.ecdh_batch(keys, peers[:2] + [(1, 1)] + peers[3:]), ("item 2", "not on the curve")),
                        (lambda: n.encrypt_batch(keys, msgs[:1] + [[0, R, 0]] + msgs[2:]), ("item 1", "message element 1")),
                        (lambda: n.encrypt_batch(keys, msgs[:3] + [[1]]), ("item 3",)),
                        (lambda: n.decrypt_batch(keys, [{"iv": 0, "msg": [0, 0, 2 * R]}] * 4), ("item 0", "ciphertext element 2")),
                        (lambda: n.ecdh_decrypt_batch(keys, peers, [{"iv": R, "msg": [0, 0, 0]}] * 4), ("item 0", "iv"))):
        with pytest.raises(zkr_hip.ZkrError) as e:
            call()
        assert e.value.code == -5 and all(w in str(e.value) for w in words), str(e.value)
    assert n.ecdh_batch([], []) == [] and n.encrypt_batch([], []) == [] and n.decrypt_batch([], []) == []
    assert n.ecdh_encrypt_batch([], [], []) == [] and n.ecdh_decrypt_batch([], [], []) == []
    L = zkr_hip.lib()
    assert L.zkr_mimc7_encrypt_batch(None, None, 5, 0, None, None, 0) == 0 and L.zkr_babyjub_ecdh_batch(None, None, 0, None, 0) == 0
