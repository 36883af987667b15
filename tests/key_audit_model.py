"""The equations of zkr_key_audit (include/zkr.h) in the exponent: every point of a key and of a transcript is
(its discrete log) x generator, so an equation between sums of points is an equation between Python integers mod r, and a pairing
equation e(a G1, b G2) == e(c G1, d G2) is a b == c d.  The logs of the key come from the oracle's setup (oracle/groth16.py
setup_scalars) for known (tau, alfa, beta, 1, delta); the transcript's are the powers themselves.  The scalar route -- row
products with rho in the witness's place, ONE inverse NTT per side, sums over the monomial basis -- is written here from the
issue's text and shares nothing with the setup's route (Lagrange basis by lagrange_at, then per-signal combinations), so the
two agreeing pins the domain, the root of unity, the inverse-NTT convention and the appended rows."""
import groth16 as g

R = g.R


def key_logs(circ, tox):
    """What an honest setup makes, as discrete logs: A, B, IC, C (None up to nPublic), hExps[0..m), alfa, beta, delta."""
    assert tox["gamma"] == 1
    sc = g.setup_scalars(circ, tox)
    return dict(n=circ["nVars"], p=circ["nPublic"], m=sc["m"], A=list(sc["a"]), B=list(sc["b"]), IC=list(sc["ic"]), C=list(sc["cpriv"]), H=list(sc["h"][:sc["m"]]),
                alfa=tox["alfa"], beta=tox["beta"], delta=tox["delta"])


def transcript_logs(tau, alfa, beta, M):
    tp = [pow(tau, i, R) for i in range(2 * M)]
    return dict(M=M, tau=tp, alfa_tau=[alfa * t % R for t in tp[:M]], beta_tau=[beta * t % R for t in tp[:M]])


def row_products(pols, v, m):
    """u[j] = sum_s pols[s][j] v_s, j < m: the prover's row product with v in the witness's place."""
    u = [0] * m
    for s, col in enumerate(pols):
        if v[s]:
            for j, cf in col.items():
                u[j] = (u[j] + cf * v[s]) % R
    return u


def coefficients(pols, v, m):
    """x(v) = iNTT_m(u(v)): sum_s v_s X_s(t) = sum_i x(v)_i t^i."""
    return g.ntt(row_products(pols, v, m), invert=True)


def dot(xs, ys):
    return sum(x * y for x, y in zip(xs, ys)) % R


def equations(circ, key, tr, rho, sigma):
    """-> {"E1": bool, ...} for the key's logs `key`, the transcript's logs `tr` and the circuit's three sides."""
    n, p, m = key["n"], key["p"], key["m"]
    assert m <= tr["M"] and len(rho) == n and len(sigma) == m
    polsA, polsB, polsC = g.qap_columns(circ)
    pub = [rho[s] if s <= p else 0 for s in range(n)]
    priv = [0 if s <= p else rho[s] for s in range(n)]

    def T(v):
        return (dot(coefficients(polsA, v, m), tr["beta_tau"]) + dot(coefficients(polsB, v, m), tr["alfa_tau"]) + dot(coefficients(polsC, v, m), tr["tau"])) % R

    a, b = coefficients(polsA, rho, m), coefficients(polsB, rho, m)
    c_sum = sum(rho[s] * key["C"][s] for s in range(p + 1, n) if key["C"][s] is not None) % R
    return {
        "E1": dot(rho, key["A"]) == dot(a, tr["tau"]),
        "E2": dot(rho, key["B"]) == dot(b, tr["tau"]),
        "E3": dot(rho, key["B"]) == dot(b, tr["tau"]),        # the same logs in G2
        "E4": dot(rho[:p + 1], key["IC"]) == T(pub),
        "E5": c_sum * key["delta"] % R == T(priv),
        "E6": dot(sigma, key["H"]) * key["delta"] % R == sum(sigma[i] * (tr["tau"][i + m] - tr["tau"][i]) for i in range(m)) % R,
    }
