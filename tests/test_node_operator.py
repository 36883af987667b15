"""GPU: the operator step from Node (index.js Ledger / Operator / txRow over napi/zkr_napi.c) against the Python Operator: one fresh
node child runs the scenario of tests/test_gpu_operator.py -- RollupCircuit(2, 3), the same toxic values, deposits, queue and
blinding -- and prints JSON; the proofs must be the same bytes.  The same child shows a refused step rejecting and leaving the root,
two steps issued without awaiting the first, save / load, and that a ledger or a Bn128 held by a live operator cannot be closed."""
import json
import os
import shutil
import subprocess

import pytest

from sequencer_model import keypair, signed_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "simple-zk-rollups_amd")
NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(os.path.join(PKG, "napi", "zkr_napi.node")),
                                                  reason="node or the N-API addon is not available")]

RS, SS = [5, 6, 7, 8], [9, 10, 11, 12]

SCRIPT = r"""
const z = require('./index.js'), fs = require('fs');
const d = JSON.parse(fs.readFileSync(process.argv[1]));
const str = (x) => JSON.parse(JSON.stringify(x, (k, v) => (typeof v === 'bigint' ? v.toString() : v)));
const brief = (r) => ({ status: r.status, consumed: r.consumed, proofs: r.batches.map((b) => b.proof), publics: r.batches.map((b) => b.publicSignals) });
(async () => {
  const out = {};
  const circuit = new z.RollupCircuit(2, 3);
  const bn = await z.buildBn128(0);
  const vk = bn.setupR1cs(circuit.r1cs(), { toxic: [2, 3, 5, 7, 11] });
  const fresh = () => { const l = new z.Ledger(3, 0); l.deposit(d.deposits.map((r) => [r[0], [r[1], r[2]], r[3], r[4]])); return l; };
  const queue = d.rows.map((r) => z.txRow(r[0], r[1], r[2], r[3], r[4], { R8: [r[5], r[6]], S: r[7] }));
  const blind = (a, b) => ({ rs: d.rs.slice(a, b), ss: d.ss.slice(a, b) });

  // the step of the Python test's first case
  const ledger = fresh();
  out.emptyRoot = ledger.root().toString();
  const op = new z.Operator({ ledger, bn, r1csBin: circuit.r1cs(), vkBin: vk, batch: 2 });
  const res = await op.step(queue, blind(0, 4));
  out.step = brief(res);
  out.solidity = res.batches[0].solidityProof;
  out.root = ledger.root().toString();
  out.info = op.info(); out.ledgerInfo = ledger.info(); out.times = op.stageTimes(); out.journal = ledger.journalInfo();
  out.account = str(ledger.account(1));
  // a ledger or a Bn128 that a live operator holds cannot be closed
  try { ledger.close(); out.closeThrew = null; } catch (e) { out.closeThrew = e.message; }
  try { bn.terminate(); out.terminateThrew = null; } catch (e) { out.terminateThrew = e.message; }
  op.close();

  // save, then load: the root is kept
  ledger.save(d.path);
  const loaded = z.Ledger.load(d.path, 0), restored = z.Ledger.restore(ledger.snapshot(), 0);
  out.loadedRoot = loaded.root().toString(); out.restoredRoot = restored.root().toString(); out.loadedInfo = loaded.info();
  loaded.close(); restored.close(); ledger.close();
  try { ledger.root(); out.closedThrew = null; } catch (e) { out.closedThrew = e.message; }

  // a verifying key of another setup: the promise rejects naming batch 0, the root stays
  const other = await z.buildBn128(0);
  const otherVk = other.setupR1cs(circuit.r1cs(), { toxic: [3, 5, 7, 11, 13] });
  other.terminate();
  const l2 = fresh();
  const bad = new z.Operator({ ledger: l2, bn, vkBin: z.binarifyVerifyingKey(otherVk), batch: 2 });
  try { await bad.step(queue, blind(0, 4)); out.rejected = null; } catch (e) { out.rejected = e.message; }
  out.rootAfterReject = l2.root().toString(); out.journalAfterReject = l2.journalInfo(); out.infoAfterReject = l2.info();
  bad.close(); l2.close();

  // two steps issued without awaiting the first, against two awaited ones
  const la = fresh(), lb = fresh();
  const a = new z.Operator({ ledger: la, bn, batch: 2 }), b = new z.Operator({ ledger: lb, bn, batch: 2 });
  const p1 = a.step(queue.slice(0, 4), blind(0, 2)), p2 = a.step(queue.slice(4), blind(2, 4));
  const got = await Promise.all([p1, p2]);
  out.unawaited = got.map(brief);
  out.awaited = [brief(await b.step(queue.slice(0, 4), blind(0, 2))), brief(await b.step(queue.slice(4), blind(2, 4)))];
  out.pairRoots = [la.root().toString(), lb.root().toString()];
  try { await a.step(queue.slice(0, 4), { rs: d.rs.slice(0, 1), ss: d.ss.slice(0, 1) }); out.shortBlinding = null; } catch (e) { out.shortBlinding = e.message; }
  a.close(); b.close(); la.close(); lb.close();
  bn.terminate();
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.fixture(scope="module")
def scenario():
    rows, nonce = [], [0] * 5
    for frm, to in ((0, 1), (1, 0), (2, 2), (3, 4), (4, 3), (0, 4), (0, 2), (3, 2)):   # the queue of tests/test_gpu_operator.py
        nonce[frm] += 1
        rows.append(signed_row(frm, to, 10, 1, nonce[frm]))
    deposits = [(i, keypair(i)[1], 1000, 0) for i in range(5)]
    return rows, deposits


@pytest.fixture(scope="module")
def python_side(scenario):
    import zkr_hip
    from zkr_hip import rollup as n
    rows, deposits = scenario
    c = n.RollupCircuit(2, 3)
    key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(c.r1cs(), toxic=[2, 3, 5, 7, 11])
    ledger = n.Ledger(3)
    ledger.deposit(deposits)
    empty_root = ledger.root
    cs = zkr_hip.ConstraintSystem.load(c.r1cs())
    with zkr_hip.VerifyingKey(vk_bin) as vk, n.Operator(ledger, key, cs, vk, batch=2) as op:
        got = op.step(rows, RS, SS)
        got["info"] = op.info()
    got.update(root=ledger.root, empty_root=empty_root, ledger_info=ledger.info(), account=ledger.account(1))
    cs.close(), ledger.close(), key.close()
    return got


@pytest.fixture(scope="module")
def node_side(scenario, tmp_path_factory):
    rows, deposits = scenario
    tmp = tmp_path_factory.mktemp("node_operator")
    args = tmp / "scenario.json"
    args.write_text(json.dumps({"rows": [[str(v) for v in r] for r in rows], "rs": [str(v) for v in RS], "ss": [str(v) for v in SS],
                                "deposits": [[i, str(pub[0]), str(pub[1]), str(bal), str(nonce)] for i, pub, bal, nonce in deposits],
                                "path": str(tmp / "ledger.bin")}))
    r = subprocess.run([NODE, "-e", SCRIPT, str(args)], cwd=PKG, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_the_node_step_equals_the_python_step(python_side, node_side):
    import zkr_hip
    py, js = python_side, node_side
    assert js["emptyRoot"] == str(py["empty_root"])
    assert js["step"]["status"] == py["status"] == [0] * 8 and js["step"]["consumed"] == py["consumed"] == 8
    assert js["step"]["proofs"] == [zkr_hip.proof_json_from_bytes(p) for p in py["proofs"]]
    assert js["step"]["publics"] == [[str(v) for v in p] for p in py["publics"]]
    assert js["root"] == str(py["root"]) and js["step"]["publics"][3][0] == js["root"]
    assert js["solidity"] == zkr_hip.solidity_proof(zkr_hip.proof_json_from_bytes(py["proofs"][0]), py["publics"][0])
    assert js["info"] == {"batch": 2, "depth": 3, "nVars": py["info"]["n_vars"], "nPublic": py["info"]["n_public"], "maxBatches": 256,
                          "deviceBytes": py["info"]["device_bytes"]}
    assert js["ledgerInfo"] == py["ledger_info"] and js["journal"] == {"checkpoints": 0, "nodes": 0}
    assert js["account"] == {"record": [str(v) for v in py["account"][0]], "path": [str(v) for v in py["account"][1]]}
    assert sorted(js["times"]) == sorted(["sequence", "witness", "check", "prove", "verify", "readOut"]) and all(v > 0 for v in js["times"].values())


def test_a_refused_step_rejects_and_leaves_the_root(python_side, node_side):
    js = node_side
    assert js["rejected"] is not None and "batch 0: proof rejected by the verifying key" in js["rejected"]
    assert js["rootAfterReject"] == str(python_side["empty_root"])
    assert js["journalAfterReject"] == {"checkpoints": 0, "nodes": 0}
    assert js["infoAfterReject"] == {"depth": 3, "accounts": 5, "applied": 0, "batches": 0}


def test_steps_issued_together_run_in_issue_order(python_side, node_side):
    import zkr_hip
    js = node_side
    assert js["unawaited"] == js["awaited"] and js["pairRoots"] == [str(python_side["root"])] * 2
    assert [len(s["proofs"]) for s in js["unawaited"]] == [2, 2]
    assert js["unawaited"][0]["proofs"] + js["unawaited"][1]["proofs"] == [zkr_hip.proof_json_from_bytes(p) for p in python_side["proofs"]]
    assert js["shortBlinding"] is not None and "blinding" in js["shortBlinding"]


def test_save_and_load_keep_the_root(python_side, node_side):
    js = node_side
    assert js["loadedRoot"] == js["restoredRoot"] == js["root"] == str(python_side["root"])
    assert js["loadedInfo"] == python_side["ledger_info"]


def test_handles_a_live_operator_holds_cannot_be_closed(node_side):
    js = node_side
    assert js["closeThrew"] is not None and "live operator" in js["closeThrew"]
    assert js["terminateThrew"] is not None and "live operator" in js["terminateThrew"]
    assert js["closedThrew"] == "the ledger is closed"
