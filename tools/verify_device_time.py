#!/usr/bin/env python3
"""Verifying a batch of proofs: the device forms against the host forms, in one call on one box.
   python tools/verify_device_time.py [--sizes 16,64,256,1024,4096] [--out profiles/verify_device_times.json]
A 73-input key (the tx circuit's count, built as tests/verify_time.py builds it: the oracle's setup at m = 2^8).  For every batch
size n, wall time of
   zkr_verify_each            proofs and signals from the host, one verdict per proof
   zkr_verify_each_device     signals read from witnesses resident on the device
   zkr_verify_batch           one host thread, one bit for the batch
   zkr_verify_batch x 8       the batch cut into eight pieces on eight host threads (the arrangement of bench.py's pipeline)
around calls that return when the answer is on the host.  The batch is 64 distinct proofs (distinct r, s over three witnesses)
repeated: no form looks at whether two proofs of a batch are equal.  Every shape is run once before it is timed; the figure is
the best of --reps runs, and the spread (worst / best) is printed beside it.  Needs a GPU: there is no CPU fallback."""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "oracle"))

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="16,64,256,1024,4096")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sizes = [int(x) for x in args.sizes.split(",")]

import groth16 as g, zkr_hip
if zkr_hip.device_count() < 1:
    sys.exit("verify_device_time.py needs a HIP device; libzkr_hip has no CPU fallback")
import torch

N_PUBLIC, DISTINCT = 73, 64
circ = g.synth_circuit(256, N_PUBLIC, 0x5A4B0001)
tox = g.toxic_from_seed(0x5A4B00FF)
_, vk = g.setup(circ, tox)
vkb = zkr_hip.binarify_verifying_key(vk)
wits = [circ["witness"]] + [g.synth_circuit(256, N_PUBLIC, 0x5A4B0001, witness_seed=500 + t)["witness"] for t in (1, 2)]
wits = [[x % g.R for x in w] for w in wits]
base_proofs = [g.proof_bytes(g.proof_from_toxic(circ, tox, wits[i % 3], 1000 + 2 * i, 2001 + 2 * i)) for i in range(DISTINCT)]
base_pubs = [wits[i % 3][1:1 + N_PUBLIC] for i in range(DISTINCT)]
d_wits = [torch.frombuffer(bytearray(g.binarify_witness(w)), dtype=torch.uint8).cuda() for w in wits]
torch.cuda.synchronize()
key = zkr_hip.VerifyingKey(vkb)
assert zkr_hip.verify(vkb, base_proofs[0], base_pubs[0])


def best_of(fn):
    fn()  # warm-up of this shape: code objects, buffers, the host verifier's key cache and its window tables
    ts = []
    for _ in range(args.reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return min(ts), max(ts) / min(ts)


def batch_in_pieces(proofs, pubs, pool):
    n = len(proofs)
    cut = [(n * k // args.threads, n * (k + 1) // args.threads) for k in range(args.threads)]
    oks = list(pool.map(lambda lh: zkr_hip.verify_batch(vkb, proofs[lh[0]:lh[1]], pubs[lh[0]:lh[1]]), [c for c in cut if c[1] > c[0]]))
    assert all(oks)


rows = []
with ThreadPoolExecutor(args.threads) as pool:
    for n in sizes:
        proofs = [base_proofs[i % DISTINCT] for i in range(n)]
        pubs = [base_pubs[i % DISTINCT] for i in range(n)]
        ptrs = [d_wits[(i % DISTINCT) % 3].data_ptr() for i in range(n)]
        forms = {
            "verify_each": lambda: key.verify_each(proofs, pubs),
            "verify_each_device": lambda: key.verify_each_device(proofs, ptrs),
            "verify_batch_1_thread": lambda: zkr_hip.verify_batch(vkb, proofs, pubs),
            "verify_batch_%d_threads" % args.threads: lambda: batch_in_pieces(proofs, pubs, pool),
        }
        assert key.verify_each(proofs, pubs) == [0] * n and key.verify_each_device(proofs, ptrs) == [0] * n
        row = {"n": n}
        for name, fn in forms.items():
            sec, spread = best_of(fn)
            row[name] = {"ms": round(1e3 * sec, 3), "proofs_per_s": round(n / sec, 1), "spread": round(spread, 3)}
            print("n %5d  %-24s %10.2f ms  %10.1f proofs/s  (worst/best %.2f)" % (n, name, 1e3 * sec, n / sec, spread), flush=True)
        rows.append(row)

host8 = "verify_batch_%d_threads" % args.threads
cross = next((r["n"] for r in rows if r["verify_each_device"]["ms"] < r[host8]["ms"]), None)
result = {"device": zkr_hip.device_pci_bus_id(0), "torch_device": torch.cuda.get_device_name(0), "date": time.strftime("%Y-%m-%d"), "n_public": N_PUBLIC,
          "reps": args.reps, "rows": rows, "crossover_vs_%d_host_threads" % args.threads: cross}
print(json.dumps(result))
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
key.close()
