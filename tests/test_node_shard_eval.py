"""The Node.js host's side of sharded proofs with H in evaluation form (napi/zkr_napi.c keyShard's sideTables, keyHForm,
shardedLastForm's hForm; index.js cachedShards): the exports on CPU, and on the GPU groth16GenProof(..., {devices}) cutting its
cached shards with side tables once the cached key has them, with unchanged proofs."""
import json
import os
import shutil
import subprocess

import pytest

import groth16 as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
NODE = shutil.which("node")
pytestmark = pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(PKG, "napi", "zkr_napi.node")),
                                reason="node or the N-API addon is not available")


def _node(script, *args):
    r = subprocess.run([NODE, "-e", script, *args], cwd=PKG, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise AssertionError(r.stderr)
    return r.stdout


def test_js_exports_and_the_addon_looks_the_new_symbols_up_optionally():
    out = _node("""
      const z = require('./index.js');
      console.log(JSON.stringify({fn: typeof z.keyHForm, stats: z.keyCacheStats().shardedLastForm}));
    """)
    res = json.loads(out)
    assert res["fn"] == "function" and res["stats"] == {"form": "none", "reason": "", "hForm": "none", "hReason": ""}
    dts = open(os.path.join(PKG, "index.d.ts")).read()
    assert 'hForm: "none" | "coefficients" | "evaluation"; hReason: string' in dts and "export function keyHForm(key: unknown)" in dts
    src = open(os.path.join(PKG, "napi", "zkr_napi.c")).read()
    for sym in ("zkr_key_shard_opts", "zkr_prove_sharded_last_h_form"):
        assert 'dlsym(h, "%s")' % sym in src   # an older library still loads


@pytest.mark.gpu
def test_js_cached_shards_take_the_side_tables_of_the_cached_key(tmp_path, small_case):
    c = small_case
    cdef = dict(nVars=c["circ"]["nVars"], nPubInputs=5, nOutputs=2,
                constraints=[[{str(s): str(cf) for s, cf in lc} for lc in row] for row in c["circ"]["rows"]])
    bad = [1] + [(x * 7 + 3) % g.R for x in c["w"][1:]]
    path, pkpath = tmp_path / "case.json", tmp_path / "pk.bin"
    pkpath.write_bytes(c["pkb"])
    path.write_text(json.dumps(dict(cdef=cdef, witness=[str(x) for x in c["w"]], bad=[str(x) for x in bad], r=str(c["r"]), s=str(c["s"]), pk=str(pkpath))))
    out = _node("""
      const z = require('./index.js'); const fs = require('fs');
      const d = JSON.parse(fs.readFileSync(process.argv[1]));
      (async () => {
        const bn = await z.buildBn128();
        const pkb = fs.readFileSync(d.pk), r1cs = z.binarifyR1cs(d.cdef), wb = z.binarifyWitness(d.witness), bad = z.binarifyWitness(d.bad);
        const opts = {r: d.r, s: d.s}, two = {r: d.r, s: d.s, devices: [0, 0]};
        const whole = await bn.groth16GenProof(wb, pkb, opts);            // a key from bytes: no side tables
        const s0 = await bn.groth16GenProof(wb, pkb, two);
        const f0 = z.shardedLastForm();
        const built = z.keyEvalTables(bn._key, r1cs), form = z.keyHForm(bn._key).form;
        const s1 = await bn.groth16GenProof(wb, pkb, two);                // a new set, cut with the tables
        const f1 = z.shardedLastForm();
        const badWhole = await bn.groth16GenProof(bad, pkb, opts);
        const badSharded = await bn.groth16GenProof(bad, pkb, two);
        const f2 = z.shardedLastForm();
        const s2 = await bn.groth16GenProof(wb, pkb, two);
        const f3 = z.shardedLastForm();
        console.log(JSON.stringify({whole, s0, s1, s2, f0, f1, f2, f3, built, form, badWhole, badSharded, shardings: z.keyCacheStats().shardings}));
      })().catch(e => { console.error(e); process.exit(1); });
    """, str(path))
    res = json.loads(out)
    want = g.proof_to_json(g.proof_from_toxic(c["circ"], c["tox"], c["w"], c["r"], c["s"]))
    assert res["whole"] == res["s0"] == res["s1"] == res["s2"] == want
    assert res["built"] is True and res["form"] == "evaluation" and res["shardings"] == 2
    assert res["f0"]["hForm"] == "coefficients" and res["f0"]["hReason"] == "shard 0 has no side tables"
    assert res["f1"]["hForm"] == "evaluation" and res["f1"]["hReason"] == "every shard has side tables" and res["f1"]["form"] == "replicated"
    assert res["badSharded"] == res["badWhole"] != want
    assert res["f2"]["hForm"] == "coefficients" and "rows unsatisfied: proved again through the coefficient form" in res["f2"]["hReason"]
    assert res["f3"]["hForm"] == "evaluation"
