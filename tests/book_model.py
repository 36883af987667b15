"""The model the book tests hold the ledger's by-key calls to (tests/test_book_cpu.py, tests/test_gpu_book.py): the contract's side
of RollUp.sol -- deposit (:255-297), withdraw / withdrawAll (:193-253), accuredFees (:139, :299-309) -- one call at a time in
Python over oracle/rollup.py's multi_hash, with the statuses and verdicts of include/zkr.h.  A dict from hashPair(publicKey) to
the account index, a set of nullifiers and the balances; the tree is sequencer_model.Model's.  Not a test module."""
import functools

import rollup as o
from sequencer_model import P250, Model

NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
HEADER = 128


@functools.lru_cache(maxsize=None)
def _hash_pair(x, y):
    return o.multi_hash([x, y])                                      # hasher.hashPair


def key_hash(pub):
    return _hash_pair(int(pub[0]), int(pub[1]))


def slot_of(nullifier, salt, mask):
    """Where the probe for a nullifier starts in a table of mask + 1 slots (include/zkr.h: a 64-bit mix of all eight words with
    the book's salt)."""
    h = salt & M64
    for i in range(8):
        h = ((h ^ ((nullifier >> (32 * i)) & 0xFFFFFFFF)) * 0x9E3779B97F4A7C15) & M64
        h ^= h >> 32
    h = ((h ^ (h >> 29)) * 0xBF58476D1CE4E5B9) & M64
    return ((h ^ (h >> 32)) & 0xFFFFFFFF) & mask


class Book:
    """balanceTreeUsers / isPublicKeysRegistered, usedNullifiers and accuredFees beside a Model."""

    def __init__(self, model=None, depth=None, cap_log2=10, nullifiers=(), fees=0):
        self.m = model if model is not None else Model(depth)
        self.nullifiers = list(nullifiers)                           # acceptance order
        self.used = set(self.nullifiers)
        self.fees = fees
        self.cap = 1 << cap_log2
        while len(self.nullifiers) > self.cap // 2:
            self.cap *= 2
        self.dirty = set()                                           # accounts whose leaf the tree has yet to see: settle()

    # ---- what the records say: the lowest index owns a key
    def users(self):
        out = {}
        for i in range(len(self.m.accounts)):
            out.setdefault(key_hash(self.m.accounts[i][:2]), i)
        return out

    def index_of(self, pubs):
        users = self.users()
        return [users.get(key_hash(p)) if p[0] < o.R and p[1] < o.R else None for p in pubs]

    def nullifiers_used(self, nullifiers):
        return [v in self.used for v in nullifiers]

    def info(self, builds):
        return {"keys": len(self.users()), "nullifiers": len(self.nullifiers), "nullifier_capacity": self.cap, "key_table_builds": builds}

    def _store(self, idx, rec):
        assert idx <= len(self.m.accounts)
        self.m.accounts[idx] = list(rec)
        self.dirty.add(idx)
        return (idx, rec[0], rec[1], rec[2], rec[3])

    def settle(self):
        """The tree is a function of the records: the leaves the calls moved are hashed once, when a list is through."""
        for idx in sorted(self.dirty):
            self.m.deposit(idx, self.m.accounts[idx][:2], self.m.accounts[idx][2], self.m.accounts[idx][3])
        self.dirty.clear()

    def _spend(self, nullifier):
        self.nullifiers.append(nullifier), self.used.add(nullifier)
        while len(self.nullifiers) > self.cap // 2:                  # the table doubles before an insert would pass half of it
            self.cap *= 2

    # ---- deposit(publicKeyX, publicKeyY) payable
    def deposit_calls(self, pubs, values):
        status, events = [], []
        users = self.users()
        for pub, value in zip(pubs, values):
            x, y = int(pub[0]), int(pub[1])
            code, ev = 0, None
            if x >= o.R or y >= o.R or value >= P250:
                code = 1
            else:
                h = key_hash((x, y))
                idx = users.get(h)
                if idx is None and len(self.m.accounts) == 1 << self.m.depth:
                    code = 2
                else:
                    rec = [x, y, 0, 0] if idx is None else list(self.m.accounts[idx])
                    if rec[2] + value >= P250:
                        code = 3
                    else:
                        rec[2] += value                              # user.balance += msg.value
                        if idx is None:
                            idx = users[h] = len(self.m.accounts)    # balanceTree.getInsertedLeavesNo()
                        ev = self._store(idx, rec)
            status.append(code), events.append(ev)
        return status, events

    # ---- withdraw / withdrawAll
    def withdraw_calls(self, publics, amounts=None, proof_verdicts=None):
        verdicts, events = [], []
        users = self.users()
        for i, sig in enumerate(publics):
            x, y, nullifier = (int(v) for v in sig)
            code, ev = 0, None
            idx = users.get(key_hash((x, y))) if x < o.R and y < o.R else None
            if x >= o.R or y >= o.R or nullifier >= o.R:
                code = 1
            elif nullifier in self.used:
                code = 2
            elif proof_verdicts is not None and proof_verdicts[i]:
                code = 3
            elif idx is None:
                code = 4
            else:
                rec = list(self.m.accounts[idx])
                amount = rec[2] if amounts is None else int(amounts[i])
                if amounts is not None and amount > rec[2]:
                    code = 5
                elif amounts is None and rec[2] == 0:
                    code = 6
                else:
                    self._spend(nullifier)                           # usedNullifiers[nullifier] = true
                    rec[2] -= amount
                    ev = self._store(idx, rec)
            verdicts.append(code), events.append(ev)
        return verdicts, events

    # ---- the blob of include/zkr.h
    def blob(self):
        return build_blob(self.nullifiers, self.fees)


def le(v, n=32):
    return int(v).to_bytes(n, "little")


def build_blob(nullifiers, fees, count=None, tag=None):
    """The ZKRBOOK1 table of include/zkr.h, byte for byte."""
    count = len(nullifiers) if count is None else count
    if tag is None:
        tag = o.multi_hash([count, fees & ((1 << 128) - 1), fees >> 128])
    return b"ZKRBOOK1" + le(count, 8) + bytes(48) + le(fees) + le(tag) + b"".join(le(v) for v in nullifiers)
