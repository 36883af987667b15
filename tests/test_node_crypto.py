"""The Node.js host's ecdh, encrypt, decrypt, ecdhEncrypt and ecdhDecrypt (simple-zk-rollups_amd/index.js over napi/zkr_napi.node,
named as in operator/src/utils/crypto.ts:86-141) against the Python host calls on three cases.  CPU only."""
import json
import os
import shutil
import subprocess

import pytest

import wallet_cases as wc
from zkr_hip import rollup as n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(PKG, "napi", "zkr_napi.node")),
                                reason="node or the N-API addon is not available")
R = n.SNARK_FIELD_SIZE

SCRIPT = """
  const z = require('./index.js');
  const cases = JSON.parse(process.argv[1]);
  const big = (v) => BigInt(v), strs = (e) => ({iv: e.iv.toString(), msg: e.msg.map(String)});
  const out = cases.map((c) => {
    const pub = c.pub.map(big), peer = c.peer.map(big), msg = c.msg.map(big);
    const key = z.ecdh(big(c.priv), peer);
    const enc = z.encrypt(msg, key), sealed = z.ecdhEncrypt(msg, big(c.priv), peer);
    return {key: key.toString(), enc: strs(enc), dec: z.decrypt(enc, key).map(String), sealed: strs(sealed),
            opened: z.ecdhDecrypt(sealed, big(c.peerPriv), pub).map(String)};
  });
  const refused = [];
  for (const f of [() => z.ecdh(1n, [1n, 1n]), () => z.encrypt([big(cases[0].r)], 1n), () => z.decrypt({iv: 0n, msg: [2n * big(cases[0].r)]}, 1n)]) {
    try { f(); refused.push(null); } catch (e) { refused.push(e.message); }
  }
  console.log(JSON.stringify({out, refused}));
"""


def test_the_five_node_calls_equal_the_python_host_calls():
    keys, pubs = wc.keys(), wc.oracle_pubs()
    (a, pa), (b, pb) = wc.kat_pairs()
    picks = [(a, pa, b, pb, [1, 2, 3]), (keys[5], pubs[5], keys[6], pubs[6], [0, R - 1, 1, 12345, R - 2]), (keys[2], pubs[2], keys[0], pubs[0], [R - 1])]
    cases = [dict(priv=str(p), pub=[str(v) for v in pp], peerPriv=str(q), peer=[str(v) for v in qp], msg=[str(v) for v in msg], r=str(R))
             for p, pp, q, qp, msg in picks]
    r = subprocess.run([NODE, "-e", SCRIPT, json.dumps(cases)], cwd=PKG, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout)
    ints = lambda e: {"iv": int(e["iv"]), "msg": [int(v) for v in e["msg"]]}
    for (p, pp, q, qp, msg), got in zip(picks, res["out"]):
        key = n.ecdh(p, qp)
        assert int(got["key"]) == key == n.ecdh(q, pp)
        assert ints(got["enc"]) == n.encrypt(msg, key) == ints(got["sealed"]) == n.ecdh_encrypt(msg, p, qp)
        assert [int(v) for v in got["dec"]] == msg == [int(v) for v in got["opened"]]
    assert all(m is not None for m in res["refused"])
    assert "not on the curve" in res["refused"][0] and "message element 0" in res["refused"][1] and "ciphertext element 0" in res["refused"][2]
