#!/usr/bin/env python3
"""One Operator.step beside the hand-written loop of INTEGRATION.md section 6.1 on the tx circuit, BatchProcessTx(2, 6): the same
queue of valid signed transactions through both, on two ledgers in one process, at 8 and at 256 batches.  profiles/operator_step.md
records a run.
   python tools/operator_time.py [--batches 8,256] [--rounds 3] [--out profiles/operator_step.md]
The loop is section 6.1 call for call (sequence, witnesses, constraint check, proofs, verify_each_device) and leaves the public
signals on the device; the step makes the same five calls inside the library, inside a ledger checkpoint, and also copies the public
signals to the host.  Per size: one untimed run of each (code objects, buffers that grow to the step), then --rounds rounds in which
the two alternate; before every run the ledger's records are put back by one deposit call, outside the timed part.  Wall time around
calls that return synchronised; Operator.stage_times() of every step beside it.  Needs a GPU: there is no CPU fallback."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import zkr_hip
from zkr_hip import rollup as n

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="8,256")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--accounts", type=int, default=64)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if zkr_hip.device_count() < 1:
    sys.exit("operator_time.py needs a HIP device; libzkr_hip has no CPU fallback")
import torch

BATCH, DEPTH = 2, 6
circuit = n.RollupCircuit(BATCH, DEPTH)
r1cs = circuit.r1cs()
t0 = time.perf_counter()
key, vk_bin = zkr_hip.ProvingKey.setup_r1cs(r1cs)
setup_s = time.perf_counter() - t0
system, vk = zkr_hip.ConstraintSystem.load(r1cs), zkr_hip.VerifyingKey(vk_bin)
privs = [0x2000 + 11 * i for i in range(a.accounts)]
pubs = n.gen_public_key_batch(privs)
deposits = [(i, pubs[i], 10 ** 9, 0) for i in range(a.accounts)]


def queue(n_txs):
    nonce, msgs = [0] * a.accounts, []
    for t in range(n_txs):
        frm, to = t % a.accounts, (7 * t + 3) % a.accounts
        nonce[frm] += 1
        msgs.append([frm, to, 1, 1, nonce[frm]])
    sigs = n.sign_batch([privs[m[0]] for m in msgs], msgs)
    return [n.tx_row(*m, s) for m, s in zip(msgs, sigs)]


def loop(ledger, rows):
    status, inputs, consumed = ledger.sequence(rows, BATCH)
    witnesses = circuit.calculate_witness_batch_from_device(inputs)
    ptrs = [witnesses[i].data_ptr() for i in range(len(witnesses))]
    ok, reports = system.check_device(ptrs)
    proofs = key.prove_batch_device(ptrs)
    verdicts = vk.verify_each_device(proofs, ptrs)
    assert ok and verdicts == [0] * len(proofs) and consumed == len(rows)
    return len(proofs)


def timed(fn, ledger):
    ledger.deposit(deposits)                           # back to the starting balances and nonces
    torch.cuda.synchronize()
    t = time.perf_counter()
    got = fn()
    return (time.perf_counter() - t) * 1e3, got


lines = []
for nb in [int(x) for x in a.batches.split(",")]:
    rows = queue(BATCH * nb)
    la, lb = n.Ledger(DEPTH), n.Ledger(DEPTH)
    op = n.Operator(lb, key, system, vk, batch=BATCH, max_batches=max(nb, 1))
    step = lambda: len(op.step(rows)["proofs"])
    assert timed(lambda: loop(la, rows), la)[1] == nb and timed(step, lb)[1] == nb      # untimed
    loop_ms, step_ms, stages = [], [], []
    for _ in range(a.rounds):
        loop_ms.append(timed(lambda: loop(la, rows), la)[0])
        step_ms.append(timed(step, lb)[0])
        stages.append(op.stage_times())
    assert la.root == lb.root
    rec = dict(batches=nb, txs=BATCH * nb, loop_ms=[round(x, 2) for x in loop_ms], step_ms=[round(x, 2) for x in step_ms],
               stage_ms=[{k: round(v, 2) for k, v in s.items()} for s in stages], device_bytes=op.info()["device_bytes"])
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    op.close(), la.close(), lb.close()

if a.out:
    spread = lambda xs: "%.2f .. %.2f (x%.2f)" % (min(xs), max(xs), max(xs) / min(xs))
    with open(a.out, "w") as f:
        f.write("# One operator step beside the hand-written loop (tools/operator_time.py)\n\n")
        f.write("BatchProcessTx(2, 6), %d accounts, a queue of valid transactions, `%s` on %s; setup %.1f s.\n" % (a.accounts, zkr_hip.version(), torch.cuda.get_device_name(0), setup_s))
        f.write("The loop and the step alternate for %d rounds after one untimed run of each; wall milliseconds, smallest .. largest of the rounds and their ratio.\n\n" % a.rounds)
        f.write("| batches | loop of section 6.1, ms | Operator.step, ms | step / loop, medians |\n|---|---|---|---|\n")
        med = lambda xs: sorted(xs)[len(xs) // 2]
        for r in lines:
            f.write("| %d | %s | %s | %.3f |\n" % (r["batches"], spread(r["loop_ms"]), spread(r["step_ms"]), med(r["step_ms"]) / med(r["loop_ms"])))
        f.write("\nStages of every timed step (`Operator.stage_times()`, ms):\n\n| batches | round | sequence | witness | check | prove | verify | read-out |\n|---|---|---|---|---|---|---|---|\n")
        for r in lines:
            for i, s in enumerate(r["stage_ms"]):
                f.write("| %d | %d | %s |\n" % (r["batches"], i, " | ".join("%.2f" % s[k] for k in n.Operator.STAGES)))
        f.write("\nRaw lines:\n\n```\n" + "\n".join(json.dumps(r) for r in lines) + "\n```\n")
