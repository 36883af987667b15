"""CPU: the scalars of the evaluation-form side tables (csrc/eval_h.hpp, through the host shim) against Python integers.

For a witness that satisfies its R1CS the H multiexp over the coefficients h equals the C' multiexp over the witness plus the E'
multiexp over the prover's coset products -- checked here on the discrete logs, where a multiexp is a dot product mod r."""
import ctypes
import os
import random

import pytest

import groth16 as g

R = g.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.environ.get("ZKR_HOSTARITH_LIB") or os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "libzkr_hostarith.so")
MONT_R = pow(2, 256, R)


@pytest.fixture(scope="module")
def shim():
    return ctypes.CDLL(SHIM)


def _b(vals):
    return b"".join(int(v % R).to_bytes(32, "little") for v in vals)


def _ints(buf, n):
    raw = bytes(buf)
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


def _circuit(m, n_public, rng, public_in_c, zero_c_column):
    """A satisfied R1CS over the domain m with c = a o b: signal 0 is one, then the public signals, then one private signal per
    constraint.  public_in_c: some C rows also carry a public signal (and the row's new signal absorbs it); zero_c_column: one
    private signal never occurs in C."""
    w = [1] + [rng.randrange(R) for _ in range(n_public)]
    rows = []
    nC = m - n_public - 1
    dead = None
    for row in range(nC):
        n = len(w)
        A = {rng.randrange(n): rng.randrange(1, R), n - 1: rng.randrange(1, R)}
        B = {rng.randrange(n): rng.randrange(1, R)}
        val = sum(cf * w[s] for s, cf in A.items()) * sum(cf * w[s] for s, cf in B.items()) % R
        if zero_c_column and row == 2:  # a * 0 = 0: the new signal is free and C never sees it
            dead = n
            rows.append((sorted(A.items()), [], []))
            w.append(rng.randrange(R))
            continue
        C = {}
        if public_in_c and row % 3 == 0:
            pub = 1 + rng.randrange(n_public)
            cf = rng.randrange(1, R)
            C[pub] = cf
            val = (val - cf * w[pub]) % R
        C[n] = 1
        rows.append((sorted(A.items()), sorted(B.items()), sorted(C.items())))
        w.append(val)
    circ = dict(nVars=len(w), nPublic=n_public, nConstraints=nC, rows=rows, witness=w, domainSize=m)
    assert g.check_r1cs(circ)
    return circ, dead


def _builder(shim, hx, logm, circ, cpriv):
    m, n, p, nC = 1 << logm, circ["nVars"], circ["nPublic"], circ["nConstraints"]
    rowC, sig, coef = [0], [], []
    for _, _, C in circ["rows"]:
        for s, cf in C:
            sig.append(s)
            coef.append(cf)
        rowC.append(len(sig))
    f, e, ep = (ctypes.create_string_buffer(32 * m) for _ in range(3))
    cfold = ctypes.create_string_buffer(32 * n)
    shim.zkt_eval_h_scalars(_b(hx), logm, (ctypes.c_uint32 * len(rowC))(*rowC), (ctypes.c_uint32 * max(1, len(sig)))(*sig), _b(coef), nC, n, p, _b(cpriv),
                            f, e, cfold, ep)
    return _ints(f, m), _ints(e, m), _ints(cfold, n), _ints(ep, m)


@pytest.mark.parametrize("logm", [3, 4])
@pytest.mark.parametrize("public_in_c,zero_c_column", [(True, False), (False, True), (True, True)])
def test_folded_scalars_reproduce_the_h_multiexp(shim, logm, public_in_c, zero_c_column):
    rng = random.Random(1000 * logm + 10 * public_in_c + zero_c_column)
    m, p = 1 << logm, 2
    circ, dead = _circuit(m, p, rng, public_in_c, zero_c_column)
    n, w = circ["nVars"], circ["witness"]
    tox = dict(t=rng.randrange(2, R), alfa=rng.randrange(1, R), beta=rng.randrange(1, R), gamma=rng.randrange(1, R), delta=rng.randrange(1, R))
    sc = g.setup_scalars(circ, tox)
    hx = [x % R for x in sc["h"][:m]]
    cpriv = [sc["cpriv"][s] % R for s in range(p + 1, n)]
    f, e, cfold, eprime = _builder(shim, hx, logm, circ, cpriv)

    # the builder's transforms are the oracle's
    assert f == g.ntt(hx, invert=True)
    gi = g.inv(g.root_of_unity(2 * m), R)
    assert e == g.ntt([hx[i] * pow(gi, i, R) % R for i in range(m)], invert=True)

    # what the prover has per proof: the coset evaluations as its unscaled inverse transforms leave them (m ao_j, m bo_j, standard
    # form) and ONE Montgomery product of the two
    pk = dict(domainSize=m, nVars=n, polsA=sc["polsA"], polsB=sc["polsB"])
    a, b = g.qap_evaluate(pk, w)
    gp = [pow(g.root_of_unity(2 * m), i, R) for i in range(m)]
    ao = g.ntt([m * x * y % R for x, y in zip(g.ntt(a, invert=True), gp)])
    bo = g.ntt([m * x * y % R for x, y in zip(g.ntt(b, invert=True), gp)])
    d = [x * y * g.inv(MONT_R, R) % R for x, y in zip(ao, bo)]

    h = g.calc_h_halves(pk, w)  # the coefficient route
    lhs = sum(hi * xi for hi, xi in zip(h, hx)) % R
    c_plain = sum(w[s] * cpriv[s - p - 1] for s in range(p + 1, n)) % R
    rhs = (sum(wi * ci for wi, ci in zip(w, cfold)) + sum(dj * ej for dj, ej in zip(d, eprime))) % R
    assert (lhs + c_plain) % R == rhs  # sum h_i hx_i + the plain C query == sum w_i cfold_i + sum d_j e'_j

    if public_in_c:  # the fold reaches the public signals, which the plain C query has no term for
        assert any(cfold[s] for s in range(1, p + 1))
    if dead is not None:  # a signal C never touches keeps its plain scalar
        assert cfold[dead] == cpriv[dead - p - 1]


@pytest.mark.parametrize("logn", [1, 3, 6])
def test_host_ntt_is_the_oracle_ntt(shim, logn):
    rng = random.Random(logn)
    x = [rng.randrange(R) for _ in range(1 << logn)]
    for inverse in (0, 1):
        buf = ctypes.create_string_buffer(_b(x), 32 << logn)
        shim.zkt_host_ntt(buf, logn, inverse)
        assert _ints(buf, 1 << logn) == g.ntt(x, invert=bool(inverse))
