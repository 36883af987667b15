#!/usr/bin/env python3
"""ecdh and the MiMC7 cipher in bulk (csrc/zkr_crypto.hip): time of each batch call on one GPU beside the same items through the
single host call on one core, in one process.   python tools/crypto_time.py [--out profiles/crypto_bulk.md] [--n 4096] [--append notes.md]

Every call is timed at the C ABI with its buffers built beforehand, by a host clock around a call that returns when its results
are on the host.  A batch call runs once as a warm-up at the same size, then `reps` times: the table gives the median (min, max).
The host call runs once in a loop over ALL n items -- the baseline: before these kernels the per-item call was the only path.
Every item of every batch result is compared byte for byte with the host loop's before a line is written.  Needs a GPU: there
is no fall-back.  --append: a file whose text is added below the table (what was not measured here: kernel resources, the
sanitizer self-check)."""
import argparse
import ctypes
import os
import random
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import torch  # noqa: E402
import zkr_hip  # noqa: E402
from zkr_hip import rollup  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crypto_bulk.md"))
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--arities", default="1,5,64")
ap.add_argument("--append", default=None)
args = ap.parse_args()
if zkr_hip.device_count() < 1:
    sys.exit("crypto_time.py needs a HIP device")
L = zkr_hip.lib()
R = rollup.SNARK_FIELD_SIZE
le = lambda v: int(v).to_bytes(32, "little")
rng = random.Random(0x5A4B000C)
n = args.n


def check(rc):
    if rc:
        raise SystemExit("zkr error %d: %s" % (rc, L.zkr_last_error().decode()))


def timed(call):
    call()   # warm-up at this size: code objects, tables, constants, allocator
    out = []
    for _ in range(args.reps):
        t = time.perf_counter()
        call()
        out.append(time.perf_counter() - t)
    return statistics.median(out), min(out), max(out)


def host_loop(call):
    t = time.perf_counter()
    for i in range(n):
        call(i)
    return time.perf_counter() - t


view = lambda buf, w, i: (ctypes.c_char * w).from_buffer(buf, w * i)
buf = lambda size: ctypes.create_string_buffer(size)
rows = []


def report(name, arity, batch_t, host_t):
    med, lo, hi = batch_t
    rows.append((name, arity, med, lo, hi, host_t))
    print("%-13s arity %2s  batch %9.3f (%9.3f .. %9.3f) ms   host %9.1f ms" % (name, arity or "-", 1e3 * med, 1e3 * lo, 1e3 * hi, 1e3 * host_t), flush=True)


def same(what, got, want):
    if bytes(got) != bytes(want):
        raise SystemExit("%s: the batch result differs from the host calls" % what)


# keys: party A's private keys meet party B's public keys, and the other way round for opening
priv_a = b"".join(le(rng.randrange(R)) for _ in range(n))
priv_b = b"".join(le(rng.randrange(R)) for _ in range(n))
pub_a, pub_b = buf(64 * n), buf(64 * n)
check(L.zkr_babyjub_pubkey_batch(priv_a, n, pub_a, 0))
check(L.zkr_babyjub_pubkey_batch(priv_b, n, pub_b, 0))
pub_a, pub_b = pub_a.raw, pub_b.raw

shared, shared_h = buf(32 * n), buf(32 * n)
bt = timed(lambda: check(L.zkr_babyjub_ecdh_batch(priv_a, pub_b, n, shared, 0)))
ht = host_loop(lambda i: check(L.zkr_babyjub_ecdh(priv_a[32 * i:32 * i + 32], pub_b[64 * i:64 * i + 64], view(shared_h, 32, i))))
same("ecdh", shared, shared_h)
report("ecdh", 0, bt, ht)
ecdh_host = ht
keys = shared_h.raw

for arity in [int(a) for a in args.arities.split(",")]:
    w = 32 * arity
    msgs = b"".join(le(rng.randrange(R)) for _ in range(n * arity))
    ivs, enc, ivs_h, enc_h, dec, dec_h = buf(32 * n), buf(w * n), buf(32 * n), buf(w * n), buf(w * n), buf(w * n)
    bt = timed(lambda: check(L.zkr_mimc7_encrypt_batch(keys, msgs, arity, n, ivs, enc, 0)))
    ht = host_loop(lambda i: check(L.zkr_mimc7_encrypt(keys[32 * i:32 * i + 32], msgs[w * i:w * i + w], arity, view(ivs_h, 32, i), view(enc_h, w, i))))
    same("encrypt", ivs.raw + enc.raw, ivs_h.raw + enc_h.raw)
    report("encrypt", arity, bt, ht)
    enc_host = ht
    ivb, encb = ivs_h.raw, enc_h.raw
    bt = timed(lambda: check(L.zkr_mimc7_decrypt_batch(keys, ivb, encb, arity, n, dec, 0)))
    ht = host_loop(lambda i: check(L.zkr_mimc7_decrypt(keys[32 * i:32 * i + 32], ivb[32 * i:32 * i + 32], encb[w * i:w * i + w], arity, view(dec_h, w, i))))
    same("decrypt", dec, dec_h)
    same("decrypt(encrypt)", dec, msgs)
    report("decrypt", arity, bt, ht)
    # the compositions: their host side is the two host calls one after the other, timed above; the results are those above
    ivs2, enc2, dec2 = buf(32 * n), buf(w * n), buf(w * n)
    bt = timed(lambda: check(L.zkr_ecdh_encrypt_batch(priv_a, pub_b, msgs, arity, n, ivs2, enc2, 0)))
    same("ecdhEncrypt", ivs2.raw + enc2.raw, ivb + encb)
    report("ecdhEncrypt", arity, bt, ecdh_host + enc_host)
    bt = timed(lambda: check(L.zkr_ecdh_decrypt_batch(priv_b, pub_a, ivb, encb, arity, n, dec2, 0)))
    same("ecdhDecrypt", dec2, msgs)
    report("ecdhDecrypt", arity, bt, ecdh_host + ht)

props = torch.cuda.get_device_properties(0)
with open(args.out, "w") as f:
    f.write("# ecdh and the MiMC7 cipher in bulk: batch call on the GPU beside the host call per item\n\n")
    f.write("`python tools/crypto_time.py`, one process on one %s (%s), n = %d items.  Batch: the whole C call (checks, upload, kernels,\n" % (props.name, zkr_hip.version(), n))
    f.write("results back on the host) under a host clock, one warm-up call, then the median (min, max) of %d calls.  Host: the same n\n" % args.reps)
    f.write("items through the single host call in a loop on one core, once -- the baseline, since the per-item call was the only path\n")
    f.write("before these kernels.  For ecdhEncrypt / ecdhDecrypt the host figure is the sum of the two host loops they are composed of.\n")
    f.write("Every item of every batch result was compared byte for byte with the host loop's before this table was written.\n\n")
    f.write("| call | arity | batch ms, median | (min, max) | items/s | elements/s | host ms for n | host us/item | host / batch |\n|---|---:|---:|---:|---:|---:|---:|---:|---:|\n")
    for name, arity, med, lo, hi, ht in rows:
        f.write("| %s | %s | %.3f | (%.3f, %.3f) | %.0f | %s | %.1f | %.1f | %.1f |\n" % (
            name, arity or "-", 1e3 * med, 1e3 * lo, 1e3 * hi, n / med, "%.0f" % (n * arity / med) if arity else "-", 1e3 * ht, 1e6 * ht / n, ht / med))
    f.write("\nNot measured: kernel time apart from the copies (the figures are whole calls), other n, more than one process, and the\nper-item calls from Node.\n")
    if args.append:
        f.write("\n" + open(args.append).read())
print("wrote", args.out)
