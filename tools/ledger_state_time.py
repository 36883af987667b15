#!/usr/bin/env python3
"""Wall times of keeping a ledger: Ledger.restore against the path a restart took before it (a fresh Ledger plus
deposit of the same records), the audit, rollback of one sequenced queue against restoring a snapshot, and zkr_ledger_sequence
with no checkpoint open against another build of the library (--parent-lib: the library of the commit before, built elsewhere)
and with one open.  Every comparison is taken inside this one process, repeats alternating.  profiles/ledger_state.md records a run.
   python tools/ledger_state_time.py [--sizes 16,20] [--txs 4096] [--repeats 3] [--parent-lib PATH]"""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-zk-rollups_amd", "python"))
import numpy as np
import torch
import zkr_hip
from zkr_hip import rollup as n

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="16,20", help="depths; each ledger is full (2^depth accounts)")
ap.add_argument("--txs", type=int, default=4096)
ap.add_argument("--accounts", type=int, default=64, help="accounts that send in the sequenced queue")
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()
L = zkr_hip.lib()
le = lambda v: int(v).to_bytes(32, "little")
ms = lambda xs: [round(x, 3) for x in xs]
median = lambda xs: sorted(xs)[len(xs) // 2]


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def random_records(count, seed):
    """count x 128 B: keys below 2^252 (< r), balances and nonces below 2^63.  No key is on the curve; nothing here signs."""
    rng = np.random.default_rng(seed)
    recs = np.zeros((count, 4, 4), dtype=np.uint64)
    recs[:, :, 0] = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    recs[:, :2, 3] = rng.integers(0, 1 << 60, size=(count, 2), dtype=np.uint64)
    return recs


def deposit_path(depth, raw, idx, count):
    """What a restart did before: a fresh ledger, then every saved record through the versioned-update path."""
    ledger = n.Ledger(depth)
    rc = L.zkr_ledger_deposit(ledger._h, idx, raw, count)
    assert rc == 0, L.zkr_last_error()
    return ledger


# ---- restore against the deposit path; the audit
for depth in [int(d) for d in a.sizes.split(",")]:
    count = 1 << depth
    raw = random_records(count, depth).tobytes()
    idx = (ctypes.c_uint32 * count).from_buffer_copy(np.arange(count, dtype=np.uint32).tobytes())
    seed = deposit_path(depth, raw, idx, count)            # warm-up of that path, and the source of the snapshot
    blob = seed.snapshot()
    check_ms = timed(lambda: n.Ledger.snapshot_check(blob))[0]
    n.Ledger.restore(blob).close()                     # warm-up
    seed.close()
    t_restore, t_deposit, t_audit = [], [], []
    for _ in range(a.repeats):                         # alternating
        dt, r = timed(lambda: n.Ledger.restore(blob))
        t_restore.append(dt)
        dt, d = timed(lambda: deposit_path(depth, raw, idx, count))
        t_deposit.append(dt)
        assert r.root == d.root and r.snapshot() == d.snapshot()
        dt, verdict = timed(r.audit)
        t_audit.append(dt)
        assert verdict is None and d.audit() is None
        r.close(), d.close()
    print(json.dumps(dict(what="restore_vs_deposit", depth=depth, accounts=count, restore_ms=ms(t_restore), deposit_path_ms=ms(t_deposit),
                          host_check_ms=round(check_ms, 3), deposit_over_restore=round(median(t_deposit) / median(t_restore), 2), audit_ms=ms(t_audit))), flush=True)

# ---- the sequencer_time.py workload at depth 16, on a full ledger whose first accounts hold real keys
depth, full = 16, 1 << 16
keys = [(0x2000 + 11 * i, n.gen_public_key(0x2000 + 11 * i)) for i in range(a.accounts)]
nonce, rows = [0] * a.accounts, []
for t in range(a.txs):
    frm, to = t % a.accounts, (7 * t + 3) % a.accounts
    nonce[frm] += 1
    rows.append(n.tx_row(frm, to, 1, 1, nonce[frm], n.sign(keys[frm][0], [frm, to, 1, 1, nonce[frm]])))
txs = b"".join(le(v) for r in rows for v in r)
senders = b"".join(le(keys[i][1][0]) + le(keys[i][1][1]) + le(10 ** 9) + le(0) for i in range(a.accounts))
sender_idx = (ctypes.c_uint32 * a.accounts)(*range(a.accounts))
rest = random_records(full, 99).tobytes()
all_idx = (ctypes.c_uint32 * full).from_buffer_copy(np.arange(full, dtype=np.uint32).tobytes())


def declare(lib):
    vp, sz, u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
    lib.zkr_last_error.restype = ctypes.c_char_p
    lib.zkr_ledger_new.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.POINTER(vp)]
    lib.zkr_ledger_free.argtypes, lib.zkr_ledger_free.restype = [vp], None
    lib.zkr_ledger_deposit.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), u8p, sz]
    lib.zkr_ledger_sequence.argtypes = [vp, u8p, sz, ctypes.c_uint32, u8p, vp, ctypes.POINTER(sz), ctypes.POINTER(sz), vp]
    return lib


class Runner:
    """One ledger of one library: reset the senders, then time zkr_ledger_sequence alone."""

    def __init__(self, lib):
        self.lib, self.h = lib, ctypes.c_void_p()
        assert lib.zkr_ledger_new(depth, 0, ctypes.byref(self.h)) == 0, lib.zkr_last_error()
        assert lib.zkr_ledger_deposit(self.h, all_idx, rest, full) == 0, lib.zkr_last_error()
        self.out = torch.empty((a.txs // a.batch, a.batch * (18 + 3 * depth) * 32), dtype=torch.uint8, device="cuda")
        self.status = ctypes.create_string_buffer(a.txs)

    def reset(self):
        assert self.lib.zkr_ledger_deposit(self.h, sender_idx, senders, a.accounts) == 0, self.lib.zkr_last_error()

    def sequence(self):
        nb, consumed = ctypes.c_size_t(), ctypes.c_size_t()
        dt, rc = timed(lambda: self.lib.zkr_ledger_sequence(self.h, txs, a.txs, a.batch, self.status, self.out.data_ptr(), ctypes.byref(nb), ctypes.byref(consumed), None))
        assert rc == 0 and self.status.raw == bytes(a.txs) and nb.value == a.txs // a.batch, (rc, self.lib.zkr_last_error())
        return dt


new = Runner(declare(ctypes.CDLL(zkr_hip.binding.LIB_PATH)))
parent = Runner(declare(ctypes.CDLL(a.parent_lib))) if a.parent_lib else None
ledger = n.Ledger._adopt(new.h, 0)                    # the same ledger through the Python host, for checkpoints and snapshots
for r in (new, parent):
    if r:
        r.reset(), r.sequence()                        # warm-up: code objects, scratch allocations
t_new, t_parent, t_open, t_rollback, t_restore = [], [], [], [], []
for _ in range(a.repeats):                             # alternating
    if parent:
        parent.reset()
        t_parent.append(parent.sequence())
    new.reset()
    t_new.append(new.sequence())
    # one checkpoint open: the same call journals first; then the rollback of that call, against restoring a snapshot
    new.reset()
    blob = ledger.snapshot()
    cp = ledger.checkpoint()
    t_open.append(new.sequence())
    nodes = ledger.journal_info()[1]
    t_rollback.append(timed(lambda: ledger.rollback(cp))[0])
    ledger.release(cp)
    assert ledger.snapshot() == blob and ledger.journal_info() == (0, 0)
    dt, other = timed(lambda: n.Ledger.restore(blob))
    t_restore.append(dt)
    assert other.root == ledger.root
    other.close()
out = dict(what="sequence_and_rollback", depth=depth, accounts=full, txs=a.txs, batch=a.batch, sequence_no_checkpoint_ms=ms(t_new),
           sequence_one_checkpoint_ms=ms(t_open), journalled_nodes=nodes, rollback_ms=ms(t_rollback), restore_snapshot_ms=ms(t_restore))
if parent:
    out.update(parent_sequence_ms=ms(t_parent), parent_spread_ms=round(max(t_parent) - min(t_parent), 3),
               new_minus_parent_median_ms=round(median(t_new) - median(t_parent), 3),
               not_above_parent_spread=bool(median(t_new) <= max(t_parent)))
print(json.dumps(out), flush=True)
