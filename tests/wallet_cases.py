"""The keys the wallet tests share (tests/test_wallet_cpu.py, tests/test_gpu_wallet.py): the edge keys, the reference's two key
pairs, one key for every length the text of multiHash([priv]) can take -- the text decides the formatted scalar and what `sign`
hashes into its nonce -- and seeded random keys to fill up.  Expected values come from oracle/rollup.py.  Not a test module."""
import functools
import json
import os
import random

import rollup as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_KEYS = 70   # one wavefront and a partial one


def text_len(priv):
    return len(o._hex_text(o.multi_hash([priv])))


@functools.lru_cache(maxsize=None)
def by_text_length():
    """{64: key, 63: key, 62: key whose text has at most 62 characters}: the first of priv = 2, 3, ... for each."""
    found = {}
    priv = 2
    while len(found) < 3:
        n = min(max(text_len(priv), 62), 64)
        found.setdefault(n, priv)
        priv += 1
        assert priv < 5000, "no key with a short hash text below 5000"
    return found


@functools.lru_cache(maxsize=None)
def keys():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "rollup_kat.json")))["keypairs"]
    out = [0, 1, o.R - 1] + [int(k["priv"]) for k in kat] + [by_text_length()[n] for n in (64, 63, 62)]
    rng = random.Random(0x5A4B000A)
    while len(out) < N_KEYS:
        out.append(rng.randrange(o.R))
    return tuple(out)


def kat_pairs():
    kat = json.load(open(os.path.join(ROOT, "tests", "golden", "rollup_kat.json")))["keypairs"]
    return [(int(k["priv"]), tuple(int(v) for v in k["pub"])) for k in kat]


@functools.lru_cache(maxsize=None)
def messages(arity):
    """One message of `arity` elements per key; the tx message (arity 5) looks like one: from to amount fee nonce."""
    rng = random.Random(0x5A4B0100 + arity)
    if arity == 5:
        return tuple((rng.randrange(4), rng.randrange(4), rng.randrange(1, 1 << 40), rng.randrange(1, 1 << 20), rng.randrange(1, 100)) for _ in keys())
    return tuple(tuple(rng.randrange(o.R) for _ in range(arity)) for _ in keys())


@functools.lru_cache(maxsize=None)
def nullifiers():
    rng = random.Random(0x5A4B0200)
    return tuple(rng.randrange(o.R) for _ in keys())


@functools.lru_cache(maxsize=None)
def oracle_formatted():
    return tuple(o.format_priv_key(k) for k in keys())


@functools.lru_cache(maxsize=None)
def oracle_pubs():
    return tuple(tuple(o.gen_public_key(k)) for k in keys())
