"""An independent model of the rest of crypto.ts for the crypto tests (tests/test_crypto_cpu.py, tests/test_gpu_crypto.py,
the curve circuit tests): circomlib's MiMC7 over the oracle's keccak-256, and ecdh / encrypt / decrypt (crypto.ts:86-141) over
the oracle's BabyJub.  Python integers only; nothing of the product.  Not a test module."""
import functools

import rollup as o

R = o.R
ROUNDS = 91


@functools.lru_cache(maxsize=None)
def constants():
    """c_0 = 0; c_i = link i of the keccak chain from keccak256("mimc"), big-endian, mod r (mimc7.js getConstants)."""
    out, h = [0], o.keccak256(b"mimc")
    for _ in range(1, ROUNDS):
        h = o.keccak256(h)
        out.append(int.from_bytes(h, "big") % R)
    return tuple(out)


def mimc7_hash(x, k):
    c, r = constants(), 0
    for i in range(ROUNDS):
        t = (x + k) % R if i == 0 else (r + k + c[i]) % R
        r = pow(t, 7, R)
    return (r + k) % R


def multi_hash(arr, key=0):
    r = key % R
    for a in arr:
        r = (r + a + mimc7_hash(a, r)) % R
    return r


def ecdh(priv, pub):   # crypto.ts:86-93
    return o.bj_mul(tuple(pub), o.format_priv_key(priv))[0]


@functools.lru_cache(maxsize=None)
def list_shared_keys():
    """ecdh of key t of tests/wallet_cases.py with the public key of key t + 1, computed once for every test that wants them
    (a tenth of a second each in Python integers)"""
    import wallet_cases as wc
    keys, pubs = wc.keys(), wc.oracle_pubs()
    return tuple(ecdh(k, pubs[(t + 1) % len(keys)]) for t, k in enumerate(keys))


def encrypt(msg, key):   # crypto.ts:95-110: BigInt `+`, not reduced
    iv = multi_hash(msg, 0)
    return {"iv": iv, "msg": [m + mimc7_hash(key, (iv + i) % R) for i, m in enumerate(msg)]}


def decrypt(enc, key):   # crypto.ts:112-123
    return [(e - mimc7_hash(key, (enc["iv"] + i) % R)) % R for i, e in enumerate(enc["msg"])]
