#!/usr/bin/env python3
"""Wall times of the ledger's book at depth 20, in one process: open_book on 2^16 accounts, 2^16 deposit calls
(half to registered keys, half to 2^13 new keys, each four times) and 2^16 withdraw calls (1 in 16 repeats a nullifier), each
beside the same effect through what the ledger offered before the book: hashPair per key on the host (zkr_mimcsponge_multihash), a
Python dict for the index and a Python set for the nullifiers, the balances in Python, then ONE event-form zkr_ledger_deposit for
the whole list.  Both sides go through the C ABI with buffers made beforehand, and end in the same root.  Writes the table, and the
registers and scratch of the new kernels (tools/kernel_resources.py), to --out.
   python tools/book_time.py [--out profiles/book.md] [--depth 20] [--log-n 16]"""
import argparse, ctypes, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import numpy as np
import torch
import zkr_hip
from zkr_hip import rollup as n

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "book.md"))
ap.add_argument("--depth", type=int, default=20)
ap.add_argument("--log-n", type=int, default=16)
a = ap.parse_args()
L = zkr_hip.lib()
N = 1 << a.log_n
le = lambda v: int(v).to_bytes(32, "little")
u32 = lambda count: (ctypes.c_uint32 * max(1, count))()


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def ok(rc):
    assert rc == 0, L.zkr_last_error()


def random_keys(count, seed):
    """count x 64 B: elements below 2^252 (< r).  No key is on the curve; nothing here signs."""
    rng = np.random.default_rng(seed)
    k = np.zeros((count, 2, 4), dtype=np.uint64)
    k[:, :, :3] = rng.integers(0, 1 << 63, size=(count, 2, 3), dtype=np.uint64)
    k[:, :, 3] = rng.integers(0, 1 << 60, size=(count, 2), dtype=np.uint64)
    return k


def host_hash(key64):
    out = ctypes.create_string_buffer(32)
    L.zkr_mimcsponge_multihash(key64, 2, out)
    return out.raw


keys = random_keys(N + N // 8, 1)
known, fresh = keys[:N], keys[N:]
records = np.zeros((N, 4, 4), dtype=np.uint64)
records[:, :2] = known
records[:, 2, 0] = 10 ** 6
raw_records = records.tobytes()
all_idx = (ctypes.c_uint32 * N).from_buffer_copy(np.arange(N, dtype=np.uint32).tobytes())
rows = []


def two_ledgers():
    book, plain = n.Ledger(a.depth), n.Ledger(a.depth)
    for x in (book, plain):
        ok(L.zkr_ledger_deposit(x._h, all_idx, raw_records, N))
    return book, plain


book, plain = two_ledgers()
warm = n.Ledger(6)                                     # code objects of the book's kernels, outside the timed calls
warm.deposit(0, (1, 2), 5), warm.open_book(), warm.deposit_calls([(1, 2)], [1]), warm.withdraw_calls([(1, 2, 3)], [1])
warm.close()

# ---- open_book beside the index a caller had to build: hashPair per record, a dict
t_open, _ = timed(lambda: book.open_book())
def host_index():
    index = {}
    for i in range(N):
        index.setdefault(host_hash(raw_records[128 * i:128 * i + 64]), i)
    return index
t_index, index = timed(host_index)
assert book.book_info()["keys"] == len(index) == N
rows.append(("open_book, 2^%d accounts" % a.log_n, t_open, "hashPair per record on the host + a dict", t_index))

# ---- deposit calls
order = np.random.default_rng(2).permutation(N)
pick = np.where(order % 2 == 0, order // 2 % N, 0)
call_keys = np.where((order % 2 == 0)[:, None, None], known[pick], fresh[(order // 2) % (N // 8)])
pubs = call_keys.tobytes()
values = np.zeros((N, 4), dtype=np.uint64)
values[:, 0] = 1 + order % 1000
values = values.tobytes()
status, idx, events = ctypes.create_string_buffer(N), u32(N), ctypes.create_string_buffer(128 * N)
t_calls, rc = timed(lambda: L.zkr_ledger_deposit_calls(book._h, pubs, values, N, status, idx, events))
ok(rc)
assert status.raw == bytes(N)


def host_deposits():
    balances, count = {}, N
    out_idx, out_rec = u32(N), bytearray(128 * N)
    for c in range(N):
        key = pubs[64 * c:64 * c + 64]
        h = host_hash(key)
        i = index.get(h)
        if i is None:
            i = index[h] = count
            count += 1
        bal = balances.get(i, 10 ** 6 if i < N else 0) + int.from_bytes(values[32 * c:32 * c + 32], "little")
        balances[i] = bal
        out_idx[c] = i
        out_rec[128 * c:128 * c + 128] = key + le(bal) + bytes(32)
    return out_idx, bytes(out_rec), balances
t_host, (h_idx, h_rec, balances) = timed(host_deposits)
t_event, rc = timed(lambda: L.zkr_ledger_deposit(plain._h, h_idx, h_rec, N))
ok(rc)
assert bytes(h_idx) == bytes(idx) and h_rec == events.raw and book.root == plain.root
rows.append(("2^%d deposit_calls" % a.log_n, t_calls, "host hashes + dict + balances (%.1f ms), one event-form deposit (%.1f ms)" % (t_host, t_event), t_host + t_event))

# ---- withdraw calls: every sixteenth repeats the nullifier in front of it
who = np.random.default_rng(3).integers(0, N, size=N)
nul = np.arange(N, dtype=np.uint64) + 10 ** 9
nul[15::16] = nul[14::16]
publics = np.zeros((N, 3, 4), dtype=np.uint64)
publics[:, :2] = known[who]
publics[:, 2, 0] = nul
publics = publics.tobytes()
amounts = np.zeros((N, 4), dtype=np.uint64)
amounts[:, 0] = 1 + who % 7
amounts = amounts.tobytes()
verdicts = ctypes.create_string_buffer(N)
t_calls, rc = timed(lambda: L.zkr_ledger_withdraw_calls(book._h, publics, amounts, None, N, verdicts, idx, events))
ok(rc)
assert verdicts.raw == (bytes(15) + b"\2") * (N // 16)


def host_withdrawals():
    used, out_idx, out_rec = set(), [], []
    for c in range(N):
        sig = publics[96 * c:96 * c + 96]
        if sig[64:] in used:
            continue
        i = index[host_hash(sig[:64])]
        amount = int.from_bytes(amounts[32 * c:32 * c + 32], "little")
        bal = balances.get(i, 10 ** 6)
        if amount > bal:
            continue
        used.add(sig[64:])
        balances[i] = bal - amount
        out_idx.append(i)
        out_rec.append(sig[:64] + le(balances[i]) + bytes(32))
    return (ctypes.c_uint32 * len(out_idx))(*out_idx), b"".join(out_rec)
t_host, (h_idx, h_rec) = timed(host_withdrawals)
t_event, rc = timed(lambda: L.zkr_ledger_deposit(plain._h, h_idx, h_rec, len(h_idx)))
ok(rc)
assert book.root == plain.root and book.book_info()["nullifiers"] == len(h_idx) == N - N // 16
rows.append(("2^%d withdraw_calls, 1 in 16 a repeat" % a.log_n, t_calls, "host hashes + dict + set + balances (%.1f ms), one event-form deposit (%.1f ms)" % (t_host, t_event), t_host + t_event))

res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "zkr_book", "--all-kernels"], capture_output=True, text=True).stdout
lines = ["# The ledger's book at depth %d: wall milliseconds, one run (tools/book_time.py)" % a.depth, "",
         "Device: %s.  Both columns were taken in one process, through the C ABI, and end in the same root." % torch.cuda.get_device_name(0), "",
         "| stage | book, ms | the same effect without the book | ms |", "|---|---:|---|---:|"]
lines += ["| %s | %.1f | %s | %.1f |" % r for r in rows]
lines += ["| total | %.1f | | %.1f |" % (sum(r[1] for r in rows), sum(r[3] for r in rows)), "",
          "Registers and scratch of the kernels of csrc/zkr_book.hip, from the compiler's metadata (tools/kernel_resources.py):", "", "```", res.rstrip(), "```", ""]
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
open(a.out, "w").write("\n".join(lines))
print("\n".join(lines))
