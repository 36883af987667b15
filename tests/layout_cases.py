"""Small rank-1 constraint systems whose keys get the chain layouts that the synthetic rollup circuit (nVars = domain size) never
gets (csrc/msm_plan.hpp proof_layout), with an oracle-made key each: for tests/test_gpu_stages.py and tests/test_gpu_shard.py."""
import functools
import random

import groth16 as g
from groth16 import R


def _case(n_vars, p, rows, w):
    circ = dict(nVars=n_vars, nPublic=p, nConstraints=len(rows), domainSize=g.domain_size(len(rows), p), rows=rows, witness=w)
    assert g.check_r1cs(circ) and len(w) == n_vars
    tox = g.toxic_from_seed(0x5A4B00FF)
    pk, _ = g.setup(circ, tox)
    return dict(circ=circ, w=w, wb=g.binarify_witness(w), pkb=g.binarify_proving_key(g.to_json_key(pk)))


@functools.lru_cache(maxsize=None)
def few_signals_many_constraints():
    """100 signals under 240 constraints: domain 2^8, so C's window (from the 100 signals) is narrower than H's (from the domain)
    and the two tables cannot share a bucket set.  94 rows make a signal each; the rest restate products of signals there are."""
    rnd = random.Random(0x5A4B0100)
    p, n_vars, n_rows = 5, 100, 240
    w = [1] + [rnd.randrange(1, R) for _ in range(p)]
    rows = []
    while len(rows) < n_rows:
        n = len(w)
        i, j, k = n - 1, rnd.randrange(n), rnd.randrange(n)
        A, B = sorted({i: 1, j: rnd.randrange(1, R)}.items()) if j != i else [(i, 1)], [(k, 1)] + ([(0, rnd.randrange(1, R))] if k else [])
        val = sum(cf * w[s] for s, cf in A) * sum(cf * w[s] for s, cf in B) % R
        if n < n_vars:
            w.append(val or 1)
            rows.append((A, B, [(n, 1)] if val else [(n, 0)]))
        else:                                           # val = coef * w_t for a signal t that is not zero
            t = next(s for s in range(rnd.randrange(n), -1, -1) if w[s])
            rows.append((A, B, [(t, val * pow(w[t], R - 2, R) % R)]))
    return _case(n_vars, p, rows, w)


@functools.lru_cache(maxsize=None)
def b_side_on_the_first_signals():
    """120 signals, domain 2^7, and a B side that reads the first eight signals only: cut into four ranges of 30 signals, the last
    three hold A and C points and no B point -- those shards reduce A in a chain of its own."""
    rnd = random.Random(0x5A4B0200)
    p, n_vars = 5, 120
    w = [1] + [rnd.randrange(1, R) for _ in range(p)]
    rows = []
    while len(w) < n_vars:
        n = len(w)
        i, j, k = n - 1, rnd.randrange(n), rnd.randrange(min(n, 8))
        A = sorted({i: 1, j: rnd.randrange(1, R)}.items()) if j != i else [(i, 1)]
        B = [(k, 1)] + ([(0, rnd.randrange(1, R))] if k else [])
        w.append(sum(cf * w[s] for s, cf in A) * sum(cf * w[s] for s, cf in B) % R)
        rows.append((A, B, [(n, 1)]))
    return _case(n_vars, p, rows, w)
