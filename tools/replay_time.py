#!/usr/bin/env python3
"""Wall time of Ledger.replay / Ledger.replay_device for the batches one Ledger.sequence call published, beside that call: the
queue of tools/sequencer_time.py (valid transactions over a few accounts), one ledger sequencing it, a second one with the same
deposits replaying the public signals from host memory and from device memory, without and with ZKR_REPLAY_SIGNATURES, each
three times and three more times with the per-stage split.  One call, one process; `--limit` ends it if something hangs.
Prints one JSON line per depth and writes them with a table to --out.  profiles/replay.md records a run.
   python tools/replay_time.py [--depths 6,16] [--txs 4096] [--accounts 64] [--batch 2] [--repeats 3] [--limit 300] [--out replay_time.md]"""
import argparse, ctypes, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import zkr_hip
from zkr_hip import rollup as n

ap = argparse.ArgumentParser()
ap.add_argument("--depths", default="6,16")
ap.add_argument("--txs", type=int, default=4096)
ap.add_argument("--accounts", type=int, default=64)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--limit", type=int, default=300, help="seconds after which the process ends itself")
ap.add_argument("--out", default="replay_time.md")
a = ap.parse_args()
signal.alarm(a.limit)
le = lambda v: int(v).to_bytes(32, "little")
L = zkr_hip.lib()

import torch
keys = [(0x2000 + 11 * i, n.gen_public_key(0x2000 + 11 * i)) for i in range(a.accounts)]
nonce, rows = [0] * a.accounts, []
for t in range(a.txs):
    frm, to = t % a.accounts, (7 * t + 3) % a.accounts
    nonce[frm] += 1
    rows.append(n.tx_row(frm, to, 1, 1, nonce[frm], n.sign(keys[frm][0], [frm, to, 1, 1, nonce[frm]])))
txs = b"".join(le(v) for r in rows for v in r)
deposits = [(i, keys[i][1], 10 ** 9, 0) for i in range(a.accounts)]
nb = a.txs // a.batch
STAGES = ("signatures", "host_pass", "leaf_hashes", "levels", "assembly")
median = lambda xs: sorted(xs)[len(xs) // 2]


def timed(ledger, call):
    """`call` on a ledger put back to the starting records, a few times plain and a few times with the stage split."""
    def run():
        ledger.deposit(deposits)                       # back to the starting balances and nonces; the scratch memory stays
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3
    os.environ.pop("ZKR_SEQUENCER_STAGES", None)
    run()                                              # warm-up: code objects, the ledger's scratch allocation
    total = [run() for _ in range(a.repeats)]
    os.environ["ZKR_SEQUENCER_STAGES"] = "1"
    staged = []
    for _ in range(a.repeats):
        t = run()
        staged.append(dict(ledger.stage_times(), total=t))
    os.environ.pop("ZKR_SEQUENCER_STAGES", None)
    return {"ms": [round(x, 3) for x in total], "staged_ms": [{k: round(v, 3) for k, v in s.items()} for s in staged]}


lines = []
for depth in [int(d) for d in a.depths.split(",")]:
    per = a.batch * (18 + 3 * depth)
    operator, follower = n.Ledger(depth), n.Ledger(depth)
    inputs = torch.empty((nb, per * 32), dtype=torch.uint8, device="cuda")
    status = ctypes.create_string_buffer(a.txs)
    c_nb, consumed = ctypes.c_size_t(), ctypes.c_size_t()

    def sequence():
        rc = L.zkr_ledger_sequence(operator._h, txs, a.txs, a.batch, status, inputs.data_ptr(), ctypes.byref(c_nb), ctypes.byref(consumed), None)
        assert rc == 0 and status.raw == bytes(a.txs) and c_nb.value == nb, (rc, L.zkr_last_error())
    out = {"depth": depth, "txs": a.txs, "accounts": a.accounts, "batch": a.batch, "sequence": timed(operator, sequence)}
    root = operator.root
    # what the operator published: word 0 of a stand-in witness is unused, then the new root (the next batch's first input, the
    # ledger's root for the last batch), then the batch's inputs
    wit = torch.zeros((nb, (2 + per) * 32), dtype=torch.uint8, device="cuda")
    wit[:, 64:] = inputs
    wit[:-1, 32:64] = inputs[1:, :32]
    wit[-1, 32:64] = torch.frombuffer(bytearray(le(root)), dtype=torch.uint8).cuda()
    publics = wit[:, 32:].contiguous().cpu().numpy().tobytes()
    ptrs = (ctypes.c_void_p * nb)(*[wit[b].data_ptr() for b in range(nb)])
    verdicts, where, applied = ctypes.create_string_buffer(nb), (ctypes.c_uint32 * nb)(), ctypes.c_size_t()
    for form, fn, first in (("replay", L.zkr_ledger_replay, publics), ("replay_device", L.zkr_ledger_replay_device, ptrs)):
        for flags in (0, n.REPLAY_SIGNATURES):
            def call():
                rc = fn(follower._h, first, nb, a.batch, None, flags, verdicts, where, ctypes.byref(applied), None)
                assert rc == 0 and verdicts.raw == bytes(nb) and applied.value == nb, (rc, L.zkr_last_error(), applied.value)
            out[form + ("_signatures" if flags else "")] = timed(follower, call)
            assert follower.root == root
    lines.append(out)
    print(json.dumps(out), flush=True)

with open(a.out, "w") as f:
    f.write("| depth | call | ms (%d repeats) | %s |\n|---|---|---|%s\n" % (a.repeats, " | ".join(STAGES), "---|" * len(STAGES)))
    for out in lines:
        for name in ("sequence", "replay", "replay_signatures", "replay_device", "replay_device_signatures"):
            r = out[name]
            f.write("| %d | %s | %s | %s |\n" % (out["depth"], name, " / ".join("%.3f" % x for x in r["ms"]),
                                                 " | ".join("%.2f" % median([s[k] for s in r["staged_ms"]]) for k in STAGES)))
    f.write("\nStage columns: medians of the staged calls.  Raw lines:\n\n```\n%s\n```\n" % "\n".join(json.dumps(o) for o in lines))
