#!/usr/bin/env python3
"""Wall time of Ledger.sequence for a queue of valid transactions, with its per-stage split, beside one host core doing the same
job with the host functions the sequencer replaces (tools/sequencer_baseline.c: zkr_eddsa_verify and the hashes of two tree
updates per transaction).  profiles/sequencer.md records a run.
   python tools/sequencer_time.py [--depths 6,16] [--txs 4096] [--accounts 64] [--batch 2] [--repeats 3]"""
import argparse, ctypes, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import zkr_hip
from zkr_hip import rollup as n
from zkr_hip.binding import LIB_PATH

ap = argparse.ArgumentParser()
ap.add_argument("--depths", default="6,16")
ap.add_argument("--txs", type=int, default=4096)
ap.add_argument("--accounts", type=int, default=64)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
le = lambda v: int(v).to_bytes(32, "little")

so = os.path.join(ROOT, "tools", "bin", "libsequencer_baseline.so")
if not os.path.exists(so):
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "sequencer_baseline.c"), "-o", so,
                           "-L" + os.path.dirname(LIB_PATH), "-lzkr_hip", "-Wl,-rpath,$ORIGIN/../../simple-zk-rollups_amd/csrc"])
L = zkr_hip.lib()
B = ctypes.CDLL(so)
B.sequencer_baseline.restype = ctypes.c_double
B.sequencer_baseline.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_size_t), ctypes.c_char_p]

import torch
keys = [(0x2000 + 11 * i, n.gen_public_key(0x2000 + 11 * i)) for i in range(a.accounts)]
nonce, rows = [0] * a.accounts, []
for t in range(a.txs):
    frm, to = t % a.accounts, (7 * t + 3) % a.accounts
    nonce[frm] += 1
    rows.append(n.tx_row(frm, to, 1, 1, nonce[frm], n.sign(keys[frm][0], [frm, to, 1, 1, nonce[frm]])))
txs = b"".join(le(v) for r in rows for v in r)
pubs = b"".join(le(keys[r[0]][1][0]) + le(keys[r[0]][1][1]) for r in rows)
deposits = [(i, keys[i][1], 10 ** 9, 0) for i in range(a.accounts)]
recs = b"".join(le(keys[i][1][0]) + le(keys[i][1][1]) + le(10 ** 9) + le(0) for r in rows for i in (r[0], r[1]))

for depth in [int(d) for d in a.depths.split(",")]:
    ledger = n.Ledger(depth)
    out = torch.empty((a.txs // a.batch, a.batch * (18 + 3 * depth) * 32), dtype=torch.uint8, device="cuda")
    status = ctypes.create_string_buffer(a.txs)
    nb, consumed = ctypes.c_size_t(), ctypes.c_size_t()

    def run():
        ledger.deposit(deposits)                       # back to the starting balances and nonces; the scratch memory stays
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.zkr_ledger_sequence(ledger._h, txs, a.txs, a.batch, status, out.data_ptr(), ctypes.byref(nb), ctypes.byref(consumed), None)
        dt = time.perf_counter() - t0
        assert rc == 0 and status.raw == bytes(a.txs) and nb.value == a.txs // a.batch, (rc, L.zkr_last_error())
        return dt * 1e3
    os.environ.pop("ZKR_SEQUENCER_STAGES", None)
    run()                                              # warm-up: code objects, the ledger's scratch allocation
    total = [run() for _ in range(a.repeats)]
    os.environ["ZKR_SEQUENCER_STAGES"] = "1"
    staged = []
    for _ in range(a.repeats):
        t = run()
        staged.append(dict(ledger.stage_times(), total=t))
    os.environ.pop("ZKR_SEQUENCER_STAGES", None)
    host = []
    for _ in range(a.repeats):
        nv, sink = ctypes.c_size_t(), ctypes.create_string_buffer(32)
        host.append(B.sequencer_baseline(txs, pubs, recs, a.txs, depth, ctypes.byref(nv), sink) * 1e3)
        assert nv.value == a.txs
    print(json.dumps(dict(depth=depth, txs=a.txs, accounts=a.accounts, batch=a.batch, sequence_ms=[round(x, 3) for x in total],
                          staged_ms=[{k: round(v, 3) for k, v in s.items()} for s in staged], host_one_core_ms=[round(x, 1) for x in host],
                          ratio_of_medians=round(sorted(host)[len(host) // 2] / sorted(total)[len(total) // 2], 1))), flush=True)
