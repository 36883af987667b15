"""The Node.js host hands back the provingKeyBin it stands in for: bn.exportKey(), bn.exportKeyJson() and keyToWebsnark(key) in one
node child, against the Python host running the same steps and against index.js's own binarifyProvingKey."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from test_gpu_contribution import _small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(PKG, "napi", "zkr_napi.node")),
                                                  reason="node or the N-API addon is not available")]
TOXIC = [0x1D0C5EED0123456789ABCDEF02468ACE13579BDF, 0x2468ACE013579BDF02468ACE13579BDF, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0, 0x5EED5EED5EED, 0x0CAFEBABEDEADBEEF0123456789ABCDEF]
D = 0x2B5C0FFEE1234567890ABCDEF0FEDCBA9876543210F00DFACE
RB, SB = 0x1234567890ABCDEF1234567890ABCDEF, 0x0FEDCBA987654321


def test_js_export_key_after_setup_and_contribution(tmp_path):
    import zkr_hip
    r1cs, wb, _, _ = _small()
    (tmp_path / "c.r1cs").write_bytes(r1cs)
    (tmp_path / "w.bin").write_bytes(wb)
    r = subprocess.run([NODE, "-e", """
      const z = require('./index.js'); const fs = require('fs'); const crypto = require('crypto');
      const sha = (ab) => crypto.createHash('sha256').update(Buffer.from(ab)).digest('hex');
      const same = (a, b) => Buffer.compare(Buffer.from(a), Buffer.from(b)) === 0;
      (async () => {
        const [r1csPath, wPath, toxic, d, r, s] = process.argv.slice(1);
        const w = fs.readFileSync(wPath);
        const bn = await z.buildBn128();
        bn.setupR1cs(fs.readFileSync(r1csPath), { toxic: JSON.parse(toxic) });
        const out = { setup: sha(bn.exportKey()), setupLen: bn.exportKey().byteLength, isArrayBuffer: bn.exportKey() instanceof ArrayBuffer };
        out.handle = same(z.keyToWebsnark(bn._key), bn.exportKey()) && same(z.keyToWebsnark(bn._key, { piecePoints: 100 }), bn.exportKey());
        bn.contribute({ d });
        const pkx = bn.exportKey({ piecePoints: 64 });
        out.contributed = sha(pkx);
        const jk = bn.exportKeyJson();
        out.json = same(z.binarifyProvingKey(JSON.parse(JSON.stringify(jk))), pkx);
        out.shape = [jk.protocol, jk.nVars, jk.nPublic, jk.domainSize, jk.domainBits, jk.C[0], jk.C.length, typeof jk.A[0][0]];
        out.held = await bn.prove(w, { r, s });
        const fresh = await z.buildBn128();
        out.fresh = await fresh.groth16GenProof(w, pkx, { r, s });
        console.log(JSON.stringify(out));
      })().catch((e) => { console.error(e); process.exit(1); });
    """, str(tmp_path / "c.r1cs"), str(tmp_path / "w.bin"), json.dumps([str(x) for x in TOXIC]), str(D), str(RB), str(SB)],
                       cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout)
    k0, _ = zkr_hip.ProvingKey.setup_r1cs(r1cs, toxic=TOXIC)
    k1, _ = k0.contribute(D)
    try:
        p0, p1 = k0.to_websnark(), k1.to_websnark()
        proof = zkr_hip.proof_json_from_bytes(k1.prove(wb, RB, SB))
    finally:
        k1.close()
        k0.close()
    assert res["isArrayBuffer"] is True and res["setupLen"] == len(p0)
    assert res["setup"] == hashlib.sha256(p0).hexdigest() and res["handle"] is True
    assert res["contributed"] == hashlib.sha256(p1).hexdigest() and p0 != p1
    assert res["json"] is True
    assert res["shape"] == ["groth", 128, 7, 128, 7, None, 128, "string"]
    strip = lambda p: {k: v for k, v in p.items() if k != "protocol"}
    assert strip(res["held"]) == proof and strip(res["fresh"]) == proof
