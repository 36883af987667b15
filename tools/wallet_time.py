#!/usr/bin/env python3
"""Keys, signatures and withdraw witnesses in bulk (csrc/zkr_wallet.hip): time of each batch call on one GPU beside the per-item
host call it replaces, in one process.   python tools/wallet_time.py [--out profiles/wallet.md] [--host-items 4096] [--reps 3]

Every call is timed at the C ABI with its buffers built beforehand, by a host clock around a call that returns when its results
are complete (the batch calls end in a copy to the host or a stream synchronise).  A batch call is timed `reps` times after one
warm-up at the same size; the table gives the fastest and the slowest.  The host call runs in a loop over the first
min(n, host-items) items and is given per item.  The batch results are compared with the host loop's before anything is written:
a table exists only for equal results.  Needs a GPU: there is no fall-back."""
import argparse
import ctypes
import os
import random
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import torch  # noqa: E402
import zkr_hip  # noqa: E402
from zkr_hip import rollup  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wallet.md"))
ap.add_argument("--host-items", type=int, default=4096)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sizes", default="64,4096,65536")
ap.add_argument("--witness-sizes", default="8,512,4096")
args = ap.parse_args()
if zkr_hip.device_count() < 1:
    sys.exit("wallet_time.py needs a HIP device")
L = zkr_hip.lib()
R = rollup.SNARK_FIELD_SIZE
ARITY = 5   # the tx message
le = lambda v: int(v).to_bytes(32, "little")
rng = random.Random(0x5A4B000A)


def check(rc):
    if rc:
        raise SystemExit("zkr error %d: %s" % (rc, L.zkr_last_error().decode()))


def timed(call, reps):
    call()   # warm-up at this size: code objects, tables, allocator
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        out.append(time.perf_counter() - t)
    return min(out), max(out)


def host_loop(call, items):
    t = time.perf_counter()
    for i in range(items):
        call(i)
    return (time.perf_counter() - t) / items


rows = []
sizes = [int(s) for s in args.sizes.split(",")]
nmax = max(sizes)
keys = [rng.randrange(R) for _ in range(nmax)]
kb = b"".join(le(k) for k in keys)
mb = b"".join(le(rng.randrange(R)) for _ in range(nmax * ARITY))
for n in sizes:
    h = min(n, args.host_items)
    out_f, out_p, out_s = (ctypes.create_string_buffer(w * n) for w in (32, 64, 96))
    one_f, one_p, one_s = (ctypes.create_string_buffer(w * h) for w in (32, 64, 96))
    view = lambda buf, w, i: (ctypes.c_char * w).from_buffer(buf, w * i)
    for name, batch, host, got, want, w in (
            ("format_privkey", lambda: check(L.zkr_babyjub_format_privkey_batch(kb, n, out_f, 0)),
             lambda i: check(L.zkr_babyjub_format_privkey(kb[32 * i:32 * i + 32], view(one_f, 32, i))), out_f, one_f, 32),
            ("pubkey", lambda: check(L.zkr_babyjub_pubkey_batch(kb, n, out_p, 0)),
             lambda i: check(L.zkr_babyjub_pubkey(kb[32 * i:32 * i + 32], view(one_p, 64, i))), out_p, one_p, 64),
            ("sign (arity 5)", lambda: check(L.zkr_eddsa_sign_batch(kb, mb, ARITY, n, out_s, 0)),
             lambda i: check(L.zkr_eddsa_sign(kb[32 * i:32 * i + 32], mb[160 * i:160 * i + 160], ARITY, view(one_s, 96, i))), out_s, one_s, 96)):
        lo, hi = timed(batch, args.reps)
        per = host_loop(host, h)
        if got.raw[:w * h] != want.raw:
            raise SystemExit("%s: the batch result differs from the host calls at n = %d" % (name, n))
        rows.append((name, n, lo, hi, per, h))
        print("%-16s n %6d  batch %9.3f .. %9.3f ms   host %8.1f us/item over %d" % (name, n, 1e3 * lo, 1e3 * hi, 1e6 * per, h), flush=True)

circ = rollup.WithdrawCircuit()
nv = circ.n_vars
wsizes = [int(s) for s in args.witness_sizes.split(",")]
wmax = max(wsizes)
fk = (ctypes.c_char * (32 * wmax))()
check(L.zkr_babyjub_format_privkey_batch(kb, wmax, fk, 0))
fkb = bytes(fk)
nb = b"".join(le(rng.randrange(R)) for _ in range(wmax))
for n in wsizes:
    h = min(n, args.host_items)
    dev = torch.empty((n, nv * 32), dtype=torch.uint8, device="cuda:0")
    lo, hi = timed(lambda: check(L.zkr_withdraw_witness_batch_device(fkb, nb, n, dev.data_ptr(), 0, None)), args.reps)
    host_w = []

    def one(i):
        p, ln = ctypes.c_void_p(), ctypes.c_size_t()
        check(L.zkr_withdraw_witness(fkb[32 * i:32 * i + 32], nb[32 * i:32 * i + 32], ctypes.byref(p), ctypes.byref(ln)))
        if i in (0, h - 1):
            host_w.append((i, ctypes.string_at(p, ln.value)))
        L.zkr_free(p)
    per = host_loop(one, h)
    for i, w in host_w:
        if bytes(dev[i].cpu().numpy()) != w:
            raise SystemExit("withdraw witness %d differs from the host builder's at n = %d" % (i, n))
    rows.append(("withdraw witness", n, lo, hi, per, h))
    print("%-16s n %6d  batch %9.3f .. %9.3f ms   host %8.1f us/item over %d" % ("withdraw witness", n, 1e3 * lo, 1e3 * hi, 1e6 * per, h), flush=True)
    del dev

props = torch.cuda.get_device_properties(0)
with open(args.out, "w") as f:
    f.write("# Keys, signatures and withdraw witnesses in bulk: batch call on the GPU beside the host call per item\n\n")
    f.write("`python tools/wallet_time.py`, one process on one %s (%s).  Batch: the whole C call (upload, kernel, result back on the host;\n" % (props.name, zkr_hip.version()))
    f.write("for witnesses: upload, kernels, stream synchronise, the witnesses stay in device memory), fastest and slowest of %d after a\n" % args.reps)
    f.write("warm-up.  Host: the per-item call in a loop over the first min(n, %d) items, per item; \"host for n\" is that times n, not a\n" % args.host_items)
    f.write("measurement of its own beyond %d items.  Results compared with the host calls before this table was written.\n\n" % args.host_items)
    f.write("| call | n | batch ms (fastest) | batch ms (slowest) | items/s (fastest) | host us/item | host for n, ms | host / batch |\n|---|---:|---:|---:|---:|---:|---:|---:|\n")
    for name, n, lo, hi, per, h in rows:
        f.write("| %s | %d | %.3f | %.3f | %.0f | %.1f | %.1f | %.1f |\n" % (name, n, 1e3 * lo, 1e3 * hi, n / lo, 1e6 * per, 1e3 * per * n, per * n / lo))
print("wrote", args.out)
