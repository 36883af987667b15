"""Host side of the reference's rollup circuit without circom / snarkjs, over the C ABI.

Mirrors /root/reference/operator/src/utils/crypto.ts (multiHash :28-30, genPublicKey :78-84, sign :143-168,
verify :170-177) and the `compiler(tx.circom)` + `Circuit.calculateWitness` steps of
operator/src/snarks/common.ts:12-21 for `BatchProcessTx(batch, depth)`
(prover/circuits/batchprocesstx.circom:3-75).  All arithmetic is native (csrc/rollup.cpp).
"""
import ctypes
import os

from .binding import BookOpts, ZkrError, _check, _take, lib

SNARK_FIELD_SIZE = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # crypto.ts:16-18
TX_INPUT_FIELDS = ("balanceTreeRoot", "txData", "txSenderPublicKey", "txSenderBalance", "txSenderNonce", "txSenderPathElements",
                   "txRecipientPublicKey", "txRecipientBalance", "txRecipientNonce", "txRecipientPathElements",
                   "intermediateBalanceTreeRoot", "intermediateBalanceTreePathElements")   # batchprocesstx.circom:13-36
REPLAY_SIGNATURES = 1   # ZKR_REPLAY_SIGNATURES


def _le(v):
    return int(v).to_bytes(32, "little")


def _ints(b):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def multi_hash(values) -> int:
    """multiHash(d) (crypto.ts:28-30); operands of any size are taken mod r as the reference's field operations do."""
    buf = b"".join(_le(int(v) % (1 << 256)) for v in values)
    assert all(0 <= int(v) < (1 << 256) for v in values)
    out = ctypes.create_string_buffer(32)
    _check(lib().zkr_mimcsponge_multihash(buf, len(values), out))
    return int.from_bytes(out.raw, "little")


def multi_hash_batch(rows, device=0):
    """multiHash of every row (equal lengths) on the GPU, one thread per hash (zkr_mimcsponge_multihash_batch)."""
    rows = [list(r) for r in rows]
    if not rows:
        return []
    arity = len(rows[0])
    assert all(len(r) == arity for r in rows)
    buf = b"".join(_le(int(v) % (1 << 256)) for r in rows for v in r)
    out = ctypes.create_string_buffer(32 * len(rows))
    _check(lib().zkr_mimcsponge_multihash_batch(buf, len(rows), arity, out, device))
    return _ints(out.raw)


def hash_left_right(left, right) -> int:   # crypto.ts:36-38
    return multi_hash([left, right])


def gen_public_key(priv):
    """genPublicKey(privKey) (crypto.ts:78-84) -> (x, y)."""
    out = ctypes.create_string_buffer(64)
    _check(lib().zkr_babyjub_pubkey(_le(priv), out))
    return tuple(_ints(out.raw))


def format_priv_key(priv) -> int:
    """formatPrivKeyForBabyJub(privKey) (crypto.ts:58-76): the scalar the circuits take as `privateKey`."""
    out = ctypes.create_string_buffer(32)
    _check(lib().zkr_babyjub_format_privkey(_le(priv), out))
    return int.from_bytes(out.raw, "little")


def sign(priv, msg):
    """sign(prv, msg) (crypto.ts:143-168) -> {"R8": (x, y), "S": s}."""
    buf = b"".join(_le(v) for v in msg)
    out = ctypes.create_string_buffer(96)
    _check(lib().zkr_eddsa_sign(_le(priv), buf, len(msg), out))
    v = _ints(out.raw)
    return {"R8": (v[0], v[1]), "S": v[2]}


def verify(msg, sig, pub) -> bool:
    """verify(msg, sig, pubKey) (crypto.ts:170-177)."""
    buf = b"".join(_le(v) for v in msg)
    sb = _le(sig["R8"][0]) + _le(sig["R8"][1]) + _le(sig["S"])
    pb = _le(pub[0]) + _le(pub[1])
    ok = ctypes.c_int()
    _check(lib().zkr_eddsa_verify(buf, len(msg), sb,
                                  pb, ctypes.byref(ok)))
    return bool(ok.value)


def verify_batch(msgs, sigs, pubs, device=0):
    """verify(msg, sig, pubKey) (crypto.ts:170-177) for many signatures on the GPU, one thread each (zkr_eddsa_verify_batch):
    msgs = equally long lists of message elements (taken mod r, as multi_hash takes them), sigs = {"R8": (x, y), "S": s},
    pubs = (x, y); elements up to 2^256 - 1.  Returns a list of bools, the answers of `verify` one by one."""
    msgs = [list(m) for m in msgs]
    n = len(msgs)
    assert len(sigs) == n and len(pubs) == n
    if n == 0:
        return []
    arity = len(msgs[0])
    assert all(len(m) == arity for m in msgs)
    mb = b"".join(_le(v) for m in msgs for v in m)
    sb = b"".join(_le(s["R8"][0]) + _le(s["R8"][1]) + _le(s["S"]) for s in sigs)
    pb = b"".join(_le(p[0]) + _le(p[1]) for p in pubs)
    out = ctypes.create_string_buffer(n)
    _check(lib().zkr_eddsa_verify_batch(mb, arity, sb, pb, n, out, device))
    return [b != 0 for b in out.raw]


def _keys_bytes(privs):
    privs = [int(p) for p in privs]
    if any(p < 0 or p >> 256 for p in privs):
        raise ValueError("a private key outside 0 .. 2^256 - 1")
    return privs, b"".join(_le(p) for p in privs)


def format_priv_key_batch(privs, device=0):
    """formatPrivKeyForBabyJub (crypto.ts:58-76) for many keys on the GPU, one thread each (zkr_babyjub_format_privkey_batch):
    a list of scalars, each what `format_priv_key` returns.  A key not below r is ZkrError(-5) naming its index."""
    privs, buf = _keys_bytes(privs)
    if not privs:
        return []
    out = ctypes.create_string_buffer(32 * len(privs))
    _check(lib().zkr_babyjub_format_privkey_batch(buf, len(privs), out, device))
    return _ints(out.raw)


def gen_public_key_batch(privs, device=0):
    """genPublicKey (crypto.ts:78-84) for many keys on the GPU (zkr_babyjub_pubkey_batch): a list of (x, y), each what
    `gen_public_key` returns."""
    privs, buf = _keys_bytes(privs)
    if not privs:
        return []
    out = ctypes.create_string_buffer(64 * len(privs))
    _check(lib().zkr_babyjub_pubkey_batch(buf, len(privs), out, device))
    v = _ints(out.raw)
    return [(v[2 * k], v[2 * k + 1]) for k in range(len(privs))]


def sign_batch(privs, msgs, device=0):
    """sign(prv, msg) (crypto.ts:143-168) for many keys and messages on the GPU (zkr_eddsa_sign_batch): msgs = equally long lists
    of message elements below r, one per key.  A list of {"R8": (x, y), "S": s}, each what `sign` returns."""
    privs, buf = _keys_bytes(privs)
    msgs = [[int(v) for v in m] for m in msgs]
    if len(msgs) != len(privs):
        raise ValueError("%d messages for %d keys" % (len(msgs), len(privs)))
    if not privs:
        return []
    arity = len(msgs[0])
    if any(len(m) != arity for m in msgs):
        raise ValueError("messages of different lengths in one batch")
    mb = b"".join(_le(v) for m in msgs for v in m)
    out = ctypes.create_string_buffer(96 * len(privs))
    _check(lib().zkr_eddsa_sign_batch(buf, mb, arity, len(privs), out, device))
    v = _ints(out.raw)
    return [{"R8": (v[3 * k], v[3 * k + 1]), "S": v[3 * k + 2]} for k in range(len(privs))]


def wallet_pubkey_program_host(priv):
    """The GPU threads' format_privkey and pubkey programs (csrc/wallet_program.hpp) on the host for one key (test hook):
    (formatted scalar, (x, y))."""
    f, p = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    _check(lib().zkr_wallet_pubkey_program_host(_le(priv), f, p))
    return int.from_bytes(f.raw, "little"), tuple(_ints(p.raw))


def wallet_sign_program_host(priv, msg):
    """The GPU threads' sign program on the host for one key and message (test hook): the dict `sign` returns."""
    out = ctypes.create_string_buffer(96)
    _check(lib().zkr_wallet_sign_program_host(_le(priv), b"".join(_le(v) for v in msg), len(msg), out))
    v = _ints(out.raw)
    return {"R8": (v[0], v[1]), "S": v[2]}


# ---- ecdh and the MiMC7 cipher (crypto.ts:86-141; csrc/zkr_crypto.hip over csrc/crypto_program.hpp)
def _les(values):
    """32-byte little-endian forms of integers in 0 .. 2^256 - 1 (what the C side then range-checks), joined."""
    values = [int(v) for v in values]
    if any(v < 0 or v >> 256 for v in values):
        raise ZkrError(-5, "a value outside 0 .. 2^256 - 1")
    return b"".join(_le(v) for v in values)


def _pubs_bytes(pubs, n):
    pubs = [tuple(p) for p in pubs]
    if len(pubs) != n or any(len(p) != 2 for p in pubs):
        raise ZkrError(-5, "%d public keys of two coordinates for %d private keys" % (len(pubs), n))
    return _les(v for p in pubs for v in p)


def _rows_bytes(rows, n, what):
    """n equally long, non-empty rows of elements -> (arity, bytes); anything else is ZkrError(-5) before a launch."""
    rows = [list(r) for r in rows]
    if len(rows) != n:
        raise ZkrError(-5, "%d %s for %d keys" % (len(rows), what, n))
    arity = len(rows[0]) if rows else 0
    for t, r in enumerate(rows):
        if len(r) != arity:
            raise ZkrError(-5, "item %d: %d elements where item 0 has %d (one arity per call)" % (t, len(r), arity))
    return arity, _les(v for r in rows for v in r)


def _encrypted_rows(ivs, buf, arity):
    v = _ints(buf)
    return [{"iv": iv, "msg": v[t * arity:(t + 1) * arity]} for t, iv in enumerate(ivs)]


def mimc7_round_constants():
    """The 91 round constants of MiMC7 as integers (zkr_mimc7_round_constants, host only); c_0 = 0."""
    out = ctypes.create_string_buffer(32 * 91)
    _check(lib().zkr_mimc7_round_constants(out))
    return _ints(out.raw)


def mimc7_hash(x, k) -> int:
    """circomlib mimc7.hash(x, k): 91 rounds of x -> x^7.  Operands not below r are ZkrError(-5)."""
    out = ctypes.create_string_buffer(32)
    _check(lib().zkr_mimc7_hash(_les([x]), _les([k]), out))
    return int.from_bytes(out.raw, "little")


def mimc7_multi_hash(values, key=0) -> int:
    """circomlib mimc7.multiHash(arr, key)."""
    values = list(values)
    out = ctypes.create_string_buffer(32)
    _check(lib().zkr_mimc7_multihash(_les(values), len(values), _les([key]), out))
    return int.from_bytes(out.raw, "little")


def ecdh(priv, pub) -> int:
    """ecdh(priv, pub) (crypto.ts:86-93): the x coordinate of formatPrivKeyForBabyJub(priv) * pub.  A public key that is not
    on the curve is ZkrError(-5): the reference multiplies whatever it is given."""
    out = ctypes.create_string_buffer(32)
    _check(lib().zkr_babyjub_ecdh(_les([priv]), _pubs_bytes([pub], 1), out))
    return int.from_bytes(out.raw, "little")


def encrypt(msg, key):
    """encrypt(msg, key) (crypto.ts:95-110) -> {"iv": int, "msg": [int, ...]}, the shape of EncryptedMessage
    (types/primitives.ts:40).  Each element is the INTEGER msg[i] + hash(key, iv + i), below 2r."""
    arity, mb = _rows_bytes([msg], 1, "messages")
    iv, out = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32 * max(arity, 1))
    _check(lib().zkr_mimc7_encrypt(_les([key]), mb, arity, iv, out))
    return _encrypted_rows(_ints(iv.raw), out.raw, arity)[0]


def decrypt(enc, key):
    """decrypt({iv, msg}, key) (crypto.ts:112-123) -> the message; ciphertext elements below 2r."""
    arity, eb = _rows_bytes([enc["msg"]], 1, "messages")
    out = ctypes.create_string_buffer(32 * max(arity, 1))
    _check(lib().zkr_mimc7_decrypt(_les([key]), _les([enc["iv"]]), eb, arity, out))
    return _ints(out.raw)[:arity]


def ecdh_encrypt(msg, priv, pub):   # crypto.ts:125-132
    return encrypt(msg, ecdh(priv, pub))


def ecdh_decrypt(enc, priv, pub):   # crypto.ts:134-141
    return decrypt(enc, ecdh(priv, pub))


def ecdh_batch(privs, pubs, device=0):
    """ecdh for many (private key, public key) pairs on the GPU, one thread each (zkr_babyjub_ecdh_batch): the shared keys,
    each what `ecdh` returns.  Refusals as `ecdh`'s, naming the first offending item, before anything is launched."""
    privs = list(privs)
    kb, pb = _les(privs), _pubs_bytes(pubs, len(privs))
    if not privs:
        return []
    out = ctypes.create_string_buffer(32 * len(privs))
    _check(lib().zkr_babyjub_ecdh_batch(kb, pb, len(privs), out, device))
    return _ints(out.raw)


def encrypt_batch(keys, msgs, device=0):
    """encrypt for many (key, message) pairs of ONE arity on the GPU (zkr_mimc7_encrypt_batch): one thread per message for the
    iv, one per message element for the keystream.  A list of {"iv", "msg"}, each what `encrypt` returns."""
    keys = list(keys)
    kb = _les(keys)
    arity, mb = _rows_bytes(msgs, len(keys), "messages")
    if not keys:
        return []
    ivs, out = ctypes.create_string_buffer(32 * len(keys)), ctypes.create_string_buffer(32 * len(keys) * max(arity, 1))
    _check(lib().zkr_mimc7_encrypt_batch(kb, mb, arity, len(keys), ivs, out, device))
    return _encrypted_rows(_ints(ivs.raw), out.raw, arity)


def decrypt_batch(keys, encs, device=0):
    """decrypt for many (key, {"iv", "msg"}) pairs of one arity on the GPU (zkr_mimc7_decrypt_batch): the messages."""
    keys, encs = list(keys), list(encs)
    kb = _les(keys)
    arity, eb = _rows_bytes([e["msg"] for e in encs], len(keys), "messages")
    ib = _les(e["iv"] for e in encs)
    if not keys:
        return []
    out = ctypes.create_string_buffer(32 * len(keys) * max(arity, 1))
    _check(lib().zkr_mimc7_decrypt_batch(kb, ib, eb, arity, len(keys), out, device))
    v = _ints(out.raw)
    return [v[t * arity:(t + 1) * arity] for t in range(len(keys))]


def ecdh_encrypt_batch(privs, pubs, msgs, device=0):
    """ecdhEncrypt (crypto.ts:125-132) for many items on the GPU (zkr_ecdh_encrypt_batch): the shared keys are computed and used
    on the device and never reach the host."""
    privs = list(privs)
    kb, pb = _les(privs), _pubs_bytes(pubs, len(privs))
    arity, mb = _rows_bytes(msgs, len(privs), "messages")
    if not privs:
        return []
    ivs, out = ctypes.create_string_buffer(32 * len(privs)), ctypes.create_string_buffer(32 * len(privs) * max(arity, 1))
    _check(lib().zkr_ecdh_encrypt_batch(kb, pb, mb, arity, len(privs), ivs, out, device))
    return _encrypted_rows(_ints(ivs.raw), out.raw, arity)


def ecdh_decrypt_batch(privs, pubs, encs, device=0):
    """ecdhDecrypt (crypto.ts:134-141) for many items on the GPU (zkr_ecdh_decrypt_batch): the messages."""
    privs, encs = list(privs), list(encs)
    kb, pb = _les(privs), _pubs_bytes(pubs, len(privs))
    arity, eb = _rows_bytes([e["msg"] for e in encs], len(privs), "messages")
    ib = _les(e["iv"] for e in encs)
    if not privs:
        return []
    out = ctypes.create_string_buffer(32 * len(privs) * max(arity, 1))
    _check(lib().zkr_ecdh_decrypt_batch(kb, pb, ib, eb, arity, len(privs), out, device))
    v = _ints(out.raw)
    return [v[t * arity:(t + 1) * arity] for t in range(len(privs))]


def tx_row(frm, to, amount, fee, nonce, sig):
    """The txData row of batchprocesstx.circom for one signed transaction: from to amount fee nonce R8x R8y S."""
    return [frm, to, amount, fee, nonce, sig["R8"][0], sig["R8"][1], sig["S"]]


def sequence_plan_host(depth, records, txs, sig_verdicts, batch):
    """The host pass of Ledger.sequence without a device (test hook, zkr_sequence_plan_host): records = [pubX, pubY, balance,
    nonce] per account, txs = tx_row lists, sig_verdicts = one truth value per transaction standing in for rule 10.
    Returns (status list, consumed, prev) with prev[table][level][update] as include/zkr.h describes the three tables."""
    n = len(txs)
    rb = b"".join(_le(v) for r in records for v in r)
    tb = b"".join(_le(v) for t in txs for v in t)
    vb = bytes(1 if v else 0 for v in sig_verdicts)
    status = ctypes.create_string_buffer(max(n, 1))
    consumed = ctypes.c_size_t()
    prev = (ctypes.c_int32 * max(1, 3 * depth * 2 * n))()
    _check(lib().zkr_sequence_plan_host(depth, rb, len(records), tb, n, vb, batch, status, ctypes.byref(consumed), prev))
    st = list(status.raw[:n])
    U = 2 * sum(1 for x in st if x == 0)
    tables = [[[prev[(t * depth + l) * U + u] for u in range(U)] for l in range(depth)] for t in range(3)]
    return st, consumed.value, tables


def _publics_bytes(publics, n_public):
    """A list of signal lists or of bytes (or one bytes object) -> (n_batches, the signals back to back)."""
    if isinstance(publics, (bytes, bytearray)):
        buf = bytes(publics)
    else:
        buf = b"".join(bytes(p) if isinstance(p, (bytes, bytearray)) else b"".join(_le(v) for v in p) for p in publics)
    if len(buf) % (32 * n_public):
        raise ValueError("public signals: %d bytes is no multiple of %d signals of 32 bytes" % (len(buf), n_public))
    return len(buf) // (32 * n_public), buf


def replay_plan_host(depth, records, publics, batch):
    """The host pass of Ledger.replay without a device (test hook, zkr_replay_plan_host): records = [pubX, pubY, balance, nonce]
    per account, publics = the signal list (or bytes) of every batch.  Returns a dict: verdicts (0 planned, 1 the first batch
    that cannot be applied, 255 behind it), where, planned, and for the planned batches' updates idx, old / new (records as
    lists of four) and tables[table][level][update] as include/zkr.h describes them."""
    n_public = 1 + batch * (18 + 3 * depth) if batch > 0 and depth > 0 else 1
    nb, pb = _publics_bytes(publics, n_public)
    rb = b"".join(_le(v) for r in records for v in r)
    room = max(1, 2 * batch * nb)
    verdicts, where = ctypes.create_string_buffer(max(nb, 1)), (ctypes.c_uint32 * max(nb, 1))()
    planned = ctypes.c_size_t()
    idx, prev = (ctypes.c_uint32 * room)(), (ctypes.c_int32 * (3 * max(depth, 1) * room))()
    old, new = ctypes.create_string_buffer(128 * room), ctypes.create_string_buffer(128 * room)
    _check(lib().zkr_replay_plan_host(depth, rb, len(records), pb, nb, batch, verdicts, where, ctypes.byref(planned), idx, old, new, prev))
    U = 2 * batch * planned.value
    recs = lambda raw: [_ints(raw[128 * u:128 * u + 128]) for u in range(U)]
    tables = [[[prev[(t * depth + l) * U + u] for u in range(U)] for l in range(depth)] for t in range(3)]
    return {"verdicts": list(verdicts.raw[:nb]), "where": list(where[:nb]), "planned": planned.value, "idx": list(idx[:U]),
            "old": recs(old.raw), "new": recs(new.raw), "tables": tables}


class Ledger:
    """The operator's state on the GPU (zkr_ledger_*): account records and the whole balance tree of `depth` levels.
    `sequence` turns a queue of signed transactions into a status each (0 accepted, 1..10 the first broken rule of
    include/zkr.h's list, 255 not reached) and the circuit inputs of every whole batch, left in device memory for
    RollupCircuit.calculate_witness_batch_from_device -- the loop of operator/src/routes/send.ts:72-135 and the tree
    updates of operator/src/routes/pubsub.ts:19-66 for a whole queue at once."""

    def __init__(self, depth, device=0):
        h = ctypes.c_void_p()
        _check(lib().zkr_ledger_new(depth, device, ctypes.byref(h)))
        self._h, self.depth, self.device = h, depth, device

    def close(self):
        if getattr(self, "_h", None):
            lib().zkr_ledger_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def deposit(self, index, pub=None, balance=None, nonce=0):
        """onEventUpdateMerkleTree (pubsub.ts:19-66): one record, or `deposit([(index, pub, balance, nonce), ...])`."""
        rows = index if pub is None else [(index, pub, balance, nonce)]
        rows = [(int(r[0]), r[1], r[2], r[3] if len(r) > 3 else 0) for r in rows]
        idx = (ctypes.c_uint32 * max(1, len(rows)))(*[r[0] for r in rows])
        buf = b"".join(_le(r[1][0]) + _le(r[1][1]) + _le(r[2]) + _le(r[3]) for r in rows)
        _check(lib().zkr_ledger_deposit(self._h, idx, buf, len(rows)))

    def info(self):
        out = (ctypes.c_uint64 * 4)()
        _check(lib().zkr_ledger_info(self._h, out))
        return {"depth": out[0], "accounts": out[1], "applied": out[2], "batches": out[3]}

    @property
    def root(self):
        out = ctypes.create_string_buffer(32)
        _check(lib().zkr_ledger_root(self._h, out))
        return int.from_bytes(out.raw, "little")

    def account(self, index):
        """-> ([pubX, pubY, balance, nonce], getUpdatePath(index).pathElements)."""
        rec, path = ctypes.create_string_buffer(128), ctypes.create_string_buffer(32 * self.depth)
        _check(lib().zkr_ledger_account(self._h, index, rec, path))
        return _ints(rec.raw), _ints(path.raw)

    def sequence(self, txs, batch, stream=None):
        """txs = tx_row lists.  -> (status list, torch.uint8 tensor [n_batches, (n_public - 1) * 32] on the device, consumed):
        row b = the inputs of batch b as RollupCircuit.flatten_inputs orders them.  The caller resubmits txs[consumed:]."""
        import torch
        n = len(txs)
        per = batch * (18 + 3 * self.depth) * 32
        buf = b"".join(_le(v) for t in txs for v in t)
        out = torch.empty((max(1, n // batch), per), dtype=torch.uint8, device=torch.device("cuda", self.device))
        status = ctypes.create_string_buffer(max(n, 1))
        nb, consumed = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().zkr_ledger_sequence(self._h, buf, n, batch, status, out.data_ptr(), ctypes.byref(nb), ctypes.byref(consumed), stream))
        return list(status.raw[:n]), out[:nb.value], consumed.value

    def _replay(self, call, first, n, batch, proof_verdicts, signatures, stream):
        if proof_verdicts is not None:
            if len(proof_verdicts) != n:
                raise ValueError("%d proof verdicts for %d batches" % (len(proof_verdicts), n))
            proof_verdicts = bytes(min(int(v), 255) for v in proof_verdicts)
        verdicts, where = ctypes.create_string_buffer(max(n, 1)), (ctypes.c_uint32 * max(n, 1))()
        applied = ctypes.c_size_t()
        _check(call(self._h, first, n, batch, proof_verdicts, REPLAY_SIGNATURES if signatures else 0, verdicts, where, ctypes.byref(applied), stream))
        return list(verdicts.raw[:n]), list(where[:n]), applied.value

    def replay(self, publics, batch, proof_verdicts=None, signatures=False, stream=None):
        """RollUp.sol:81-161 for a run of consecutive published batches against this ledger (zkr_ledger_replay): publics = the
        public signals of every batch as a list of signal lists or of bytes (circom's order, newBalanceTreeRoot first),
        proof_verdicts = what VerifyingKey.verify_each returned for them, or None; signatures=True also checks every
        transaction's signature under the sender's stored key.  -> (verdicts, where, applied): 0 applied, 1 cannot be applied,
        2 not the current root, 3 the proof is refused, 5 a signature fails, 4 a signal differs from what the ledger derives,
        255 behind the first refused batch; include/zkr.h says what `where` names for each.  The ledger ends as it stands
        after the last batch with verdict 0."""
        n, buf = _publics_bytes(publics, 1 + batch * (18 + 3 * self.depth))
        return self._replay(lib().zkr_ledger_replay, buf, n, batch, proof_verdicts, signatures, stream)

    def replay_device(self, witness_ptrs, batch, proof_verdicts=None, signatures=False, stream=None):
        """The same with the signals read in place (zkr_ledger_replay_device): witness_ptrs = one device pointer per batch, the
        batch's signals are words 1..n_public of that witness -- the convention of VerifyingKey.verify_each_device."""
        n = len(witness_ptrs)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in witness_ptrs])
        return self._replay(lib().zkr_ledger_replay_device, ptrs, n, batch, proof_verdicts, signatures, stream)

    def stage_times(self):
        """Milliseconds of the last sequence or replay call's stages (recorded only with ZKR_SEQUENCER_STAGES set in the
        environment).  For a replay "signatures" includes the signals' way to the device (or back from it) and "assembly" is
        the comparison and the store."""
        out = (ctypes.c_double * 5)()
        _check(lib().zkr_ledger_stage_times(self._h, out))
        return dict(zip(("signatures", "host_pass", "leaf_hashes", "levels", "assembly"), out))

    # ---- keeping the ledger (include/zkr.h)
    @classmethod
    def _adopt(cls, handle, device):
        self = cls.__new__(cls)
        self._h, self.device = handle, device
        try:
            self.depth = self.info()["depth"]
        except Exception:
            self.close()
            raise
        return self

    def records(self, first=0, count=None):
        """[pubX, pubY, balance, nonce] of `count` accounts from `first` on (default: all), from the host copy."""
        if count is None:
            count = self.info()["accounts"] - first
        out = ctypes.create_string_buffer(max(1, 128 * count))
        _check(lib().zkr_ledger_records(self._h, first, count, out))
        return [_ints(out.raw[128 * i:128 * i + 128]) for i in range(count)]

    def tree(self):
        """The stored tree as a zero-copy torch uint8 view of device memory, [2^(depth+1) - 1, 32]: leaves first, root last,
        standard form.  Read-only by contract; valid while the ledger lives; its contents move with every state-changing call."""
        from .batch import _tensor_from_ptr
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_ledger_tree(self._h, ctypes.byref(p), ctypes.byref(n)))
        return _tensor_from_ptr(p.value, n.value, self.device).view(-1, 32)

    def paths(self, indices):
        """getUpdatePath(i).pathElements for every i of `indices`, gathered from the tree view in one go."""
        import torch
        indices = [int(i) for i in indices]
        if any(i < 0 or i >> self.depth for i in indices):
            raise ValueError("a leaf index outside the tree of depth %d" % self.depth)
        if not indices:
            return []
        rows = [((2 << self.depth) - (2 << (self.depth - l))) + ((i >> l) ^ 1) for i in indices for l in range(self.depth)]
        view = self.tree()
        got = view[torch.tensor(rows, dtype=torch.int64, device=view.device)].cpu().numpy().tobytes()
        vals = _ints(got)
        return [vals[k * self.depth:(k + 1) * self.depth] for k in range(len(indices))]

    def snapshot(self) -> bytes:
        """The ZKRLEDG1 blob of the current state: a header pinned by its tag, the records pinned by the root."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_ledger_snapshot(self._h, ctypes.byref(p), ctypes.byref(n)))
        return _take(p, n.value)

    def save(self, path):
        _check(lib().zkr_ledger_save(self._h, os.fsencode(path)))

    @staticmethod
    def snapshot_check(blob):
        """Host only: (info dict, None) of a well-formed blob, or (None, the line naming the first failure)."""
        blob = bytes(blob)
        info, valid = (ctypes.c_uint64 * 4)(), ctypes.c_int()
        _check(lib().zkr_ledger_snapshot_check(blob, len(blob), info, ctypes.byref(valid)))
        if not valid.value:
            return None, lib().zkr_last_error().decode()
        return {"depth": info[0], "accounts": info[1], "applied": info[2], "batches": info[3]}, None

    @classmethod
    def restore(cls, blob, device=0):
        """A new ledger from a snapshot: checked on the host (ZkrError -5), rebuilt in bulk on the device, and refused
        (ZkrError -2, both roots in the message) when the records do not rebuild to the snapshot's root."""
        blob = bytes(blob)
        h = ctypes.c_void_p()
        _check(lib().zkr_ledger_restore(blob, len(blob), device, ctypes.byref(h)))
        return cls._adopt(h, device)

    @classmethod
    def load(cls, path, device=0):
        h = ctypes.c_void_p()
        _check(lib().zkr_ledger_load_file(os.fsencode(path), device, ctypes.byref(h)))
        return cls._adopt(h, device)

    def checkpoint(self) -> int:
        """Opens a checkpoint and returns its id.  Until every checkpoint is released, each storing call journals what it
        overwrites, so that `rollback(cp)` puts records, tree and counters back exactly as they stand now."""
        cp = ctypes.c_uint64()
        _check(lib().zkr_ledger_checkpoint(self._h, ctypes.byref(cp)))
        return cp.value

    def rollback(self, cp):
        _check(lib().zkr_ledger_rollback(self._h, cp))

    def release(self, cp):
        _check(lib().zkr_ledger_release(self._h, cp))

    def journal_info(self):
        """(open checkpoints, journalled nodes)."""
        out = (ctypes.c_uint64 * 2)()
        _check(lib().zkr_ledger_journal_info(self._h, out))
        return out[0], out[1]

    def audit(self):
        """None when the stored tree is the tree of the records, else (level, index) of the first node that is not."""
        report, sound = (ctypes.c_uint64 * 2)(), ctypes.c_int()
        _check(lib().zkr_ledger_audit(self._h, report, ctypes.byref(sound)))
        return None if sound.value else (report[0], report[1])


    # ---- the book: the contract's side, by public key (include/zkr.h)
    def open_book(self, blob=None, nullifier_cap_log2=None, salt=None):
        """Opens the ledger's book (zkr_ledger_book_open): the key table over the records, the nullifier set (empty, or the one
        of a ZKRBOOK1 `blob` from book_blob) and the fee counter.  nullifier_cap_log2: the set's first table size (default 10);
        salt: the 64-bit value that places nullifiers in their table (default: drawn from the OS)."""
        opts = BookOpts(int(nullifier_cap_log2 or 0), 0, int(salt or 0))
        blob = None if blob is None else bytes(blob)
        _check(lib().zkr_ledger_book_open(self._h, ctypes.byref(opts), blob, len(blob) if blob is not None else 0))

    def book_info(self):
        out = (ctypes.c_uint64 * 4)()
        _check(lib().zkr_ledger_book_info(self._h, out))
        return {"keys": out[0], "nullifiers": out[1], "nullifier_capacity": out[2], "key_table_builds": out[3]}

    @staticmethod
    def _events(n, codes, indices, events):
        """One (index, pubX, pubY, balance, nonce) per applied call -- the contract's event -- and None per refused one."""
        codes = list(codes.raw[:n])
        return codes, [None if codes[i] else tuple([indices[i]] + _ints(events.raw[128 * i:128 * i + 128])) for i in range(n)]

    def deposit_calls(self, pubs, values):
        """deposit(publicKeyX, publicKeyY) payable (RollUp.sol:255-297) for a list of calls in order: pubs = (x, y) pairs,
        values = msg.value each.  -> (status, events): status 0 applied, 1 out of range, 2 tree full, 3 balance past 2^250;
        events[i] = the Deposit event (index, pubX, pubY, balance, nonce) of an applied call, None of a refused one."""
        n = len(pubs)
        if len(values) != n:
            raise ValueError("%d values for %d deposit calls" % (len(values), n))
        pb, vb = b"".join(_le(p[0]) + _le(p[1]) for p in pubs), b"".join(_le(v) for v in values)
        status, idx, ev = ctypes.create_string_buffer(max(n, 1)), (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(128 * max(n, 1))
        _check(lib().zkr_ledger_deposit_calls(self._h, pb, vb, n, status, idx, ev))
        return self._events(n, status, idx, ev)

    @staticmethod
    def _withdraw_args(n, amounts, proof_verdicts):
        if amounts is not None and len(amounts) != n:
            raise ValueError("%d amounts for %d withdraw calls" % (len(amounts), n))
        if proof_verdicts is not None and len(proof_verdicts) != n:
            raise ValueError("%d proof verdicts for %d withdraw calls" % (len(proof_verdicts), n))
        ab = None if amounts is None else b"".join(int(a).to_bytes(32, "little") for a in amounts)
        vb = None if proof_verdicts is None else bytes(min(int(v), 255) for v in proof_verdicts)
        return ab, vb, ctypes.create_string_buffer(max(n, 1)), (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(128 * max(n, 1))

    def withdraw_calls(self, publics, amounts=None, proof_verdicts=None):
        """withdraw (RollUp.sol:212-253) for a list of calls in order, or withdrawAll (:193-210) for every call when amounts is
        None.  publics = [pubX, pubY, nullifier] per call, proof_verdicts = what VerifyingKey.verify_each returned, or None.
        -> (verdicts, events): 0 applied, 1 a signal not below r, 2 nullifier used, 3 proof refused, 4 key not registered,
        5 amount above the balance, 6 withdrawAll of a zero balance; events[i] = the Withdraw event or None."""
        n = len(publics)
        ab, vb, verdicts, idx, ev = self._withdraw_args(n, amounts, proof_verdicts)
        pb = b"".join(_le(p[0]) + _le(p[1]) + _le(p[2]) for p in publics)
        _check(lib().zkr_ledger_withdraw_calls(self._h, pb, ab, vb, n, verdicts, idx, ev))
        return self._events(n, verdicts, idx, ev)

    def withdraw_calls_device(self, witness_ptrs, amounts=None, proof_verdicts=None, stream=None):
        """The same with the signals read in place (zkr_ledger_withdraw_calls_device): witness_ptrs = one device pointer per
        call, its signals are words 1..3 of that witness -- the convention of VerifyingKey.verify_each_device."""
        n = len(witness_ptrs)
        ab, vb, verdicts, idx, ev = self._withdraw_args(n, amounts, proof_verdicts)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[int(p) for p in witness_ptrs])
        _check(lib().zkr_ledger_withdraw_calls_device(self._h, ptrs, ab, vb, n, verdicts, idx, ev, stream))
        return self._events(n, verdicts, idx, ev)

    def index_of(self, pubs):
        """The account that owns each (x, y) key, None where the key is not registered."""
        n = len(pubs)
        out = (ctypes.c_uint32 * max(n, 1))()
        _check(lib().zkr_ledger_lookup_keys(self._h, b"".join(_le(p[0]) + _le(p[1]) for p in pubs), n, out))
        return [None if out[i] == 0xFFFFFFFF else out[i] for i in range(n)]

    def nullifiers_used(self, nullifiers):
        n = len(nullifiers)
        out = ctypes.create_string_buffer(max(n, 1))
        _check(lib().zkr_ledger_nullifiers_used(self._h, b"".join(_le(v) for v in nullifiers), n, out))
        return [bool(v) for v in out.raw[:n]]

    def fees(self, reset=False):
        """accuredFees (RollUp.sol:139, :299-309): the fees of every transaction applied while the book is open; reset=True
        also zeroes the counter, as withdrawAccuredFees does."""
        out = ctypes.create_string_buffer(32)
        _check(lib().zkr_ledger_fees(self._h, out, 1 if reset else 0))
        return int.from_bytes(out.raw, "little")

    def book_blob(self) -> bytes:
        """The ZKRBOOK1 blob of the book: nullifier count, fees, a tag over both, the nullifiers in acceptance order."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_ledger_book_blob(self._h, ctypes.byref(p), ctypes.byref(n)))
        return _take(p, n.value)

    @staticmethod
    def book_blob_check(blob):
        """Host only: ({"nullifiers", "fees"}, None) of a well-formed blob, or (None, the line naming the first failure)."""
        blob = bytes(blob)
        info, valid = (ctypes.c_uint64 * 2)(), ctypes.c_int()
        _check(lib().zkr_book_blob_check(blob, len(blob), info, ctypes.byref(valid)))
        if not valid.value:
            return None, lib().zkr_last_error().decode()
        return {"nullifiers": info[0], "fees": int.from_bytes(blob[64:96], "little")}, None


class Operator:
    """One operator step behind one handle (zkr_operator_*): `step` takes a queue of signed transactions and returns
    statuses, proofs and public signals -- Ledger.sequence, RollupCircuit.calculate_witness_batch_from_device,
    ConstraintSystem.check_device, ProvingKey.prove_batch_device and VerifyingKey.verify_each_device in that order, over device
    buffers the handle owns, inside a ledger checkpoint of its own: the ledger moves only when every proof of the step is good.
    ledger, key, system (a ConstraintSystem, or None: no constraint check) and vk (a VerifyingKey, or None: no acceptance check --
    verify_each_device takes about 50 ms whatever the batch size; check on the host with zkr_hip.verify_batch instead) are borrowed
    and must outlive the operator, which keeps references to them.  A mismatch between them is ZkrError(-5) naming it."""
    STAGES = ("sequence", "witness", "check", "prove", "verify", "read_out")

    def __init__(self, ledger, key, system=None, vk=None, batch=2, max_batches=None):
        from .binding import OperatorOpts
        self._h = None
        self._held = (ledger, key, system, vk)
        self.batch = int(batch)
        opts = OperatorOpts(self.batch, int(max_batches or 0), 0, 0)
        h = ctypes.c_void_p()
        _check(lib().zkr_operator_new(ledger._h, key._h, system._h if system is not None else None, vk._h if vk is not None else None,
                                      ctypes.byref(opts), ctypes.byref(h)))
        self._h = h
        self.n_public = self.info()["n_public"]

    def step(self, txs, rs=None, ss=None):
        """txs = tx_row lists; rs / ss = one blinding scalar per batch the queue can fill (len(txs) // batch), or None: drawn per
        proof.  -> {"status": one code per transaction as Ledger.sequence gives them, "consumed": the caller resubmits
        txs[consumed:], "proofs": [256 bytes per batch], "publics": [the n_public signals of each batch]}.  Raises ZkrError with
        the ledger as it was before the call when a witness, a constraint, a proof or the verifying key refuses a batch."""
        from .binding import _blinding_bytes
        n = len(txs)
        room = n // self.batch
        rb, sb = _blinding_bytes(rs, ss, room)   # a short list must not reach the C side
        buf = b"".join(_le(v) for t in txs for v in t)
        status = ctypes.create_string_buffer(max(n, 1))
        proofs = ctypes.create_string_buffer(max(256 * room, 1))
        publics = ctypes.create_string_buffer(max(32 * self.n_public * room, 1))
        nb, consumed = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().zkr_operator_step(self._h, buf, n, rb, sb, status, proofs, publics, ctypes.byref(nb), ctypes.byref(consumed)))
        row = 32 * self.n_public
        return {"status": list(status.raw[:n]), "consumed": consumed.value,
                "proofs": [proofs.raw[256 * b:256 * b + 256] for b in range(nb.value)],
                "publics": [_ints(publics.raw[row * b:row * b + row]) for b in range(nb.value)]}

    def info(self):
        out = (ctypes.c_uint64 * 6)()
        _check(lib().zkr_operator_info(self._h, out))
        return dict(zip(("batch", "depth", "n_vars", "n_public", "max_batches", "device_bytes"), (int(v) for v in out)))

    def stage_times(self):
        """Wall milliseconds of the last step's stages (0 for a stage that did not run)."""
        out = (ctypes.c_double * 6)()
        _check(lib().zkr_operator_stage_times(self._h, out))
        return dict(zip(self.STAGES, out))

    def close(self):
        if getattr(self, "_h", None):
            lib().zkr_operator_free(self._h)
            self._h = None
        self._held = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _resolved_words(resolved):
    flat = [int(w) for r in resolved for w in r]
    return (ctypes.c_uint32 * max(1, len(flat)))(*flat)


def book_deposit_plan_host(depth, records, pubs, values, resolved):
    """The host pass of Ledger.deposit_calls without a device (test hook, zkr_book_deposit_plan_host): resolved = (flags, account,
    leader) per call as include/zkr.h describes them.  -> (status, events) as Ledger.deposit_calls returns them."""
    n = len(pubs)
    rb = b"".join(_le(v) for r in records for v in r)
    status, idx, ev = ctypes.create_string_buffer(max(n, 1)), (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(128 * max(n, 1))
    _check(lib().zkr_book_deposit_plan_host(depth, rb, len(records), b"".join(_le(p[0]) + _le(p[1]) for p in pubs), b"".join(_le(v) for v in values), n,
                                            _resolved_words(resolved), status, idx, ev))
    return Ledger._events(n, status, idx, ev)


def book_withdraw_plan_host(records, publics, amounts, proof_verdicts, resolved):
    """The host pass of Ledger.withdraw_calls without a device (test hook, zkr_book_withdraw_plan_host)."""
    n = len(publics)
    rb = b"".join(_le(v) for r in records for v in r)
    ab, vb, verdicts, idx, ev = Ledger._withdraw_args(n, amounts, proof_verdicts)
    _check(lib().zkr_book_withdraw_plan_host(rb, len(records), b"".join(_le(p[0]) + _le(p[1]) + _le(p[2]) for p in publics), ab, vb, n,
                                             _resolved_words(resolved), verdicts, idx, ev))
    return Ledger._events(n, verdicts, idx, ev)


class RollupCircuit:
    """BatchProcessTx(batch, depth): what `new Circuit(await compiler("tx.circom"))` is to the reference
    (common.ts:12-15).  `r1cs()` feeds ProvingKey.setup_r1cs; `calculate_witness(inputs)` returns the witness as
    binarifyWitness would lay it out (nVars x 32 B) and raises ZkrError(-7) where calculateWitness would throw."""

    def __init__(self, batch=2, depth=6):   # tx.circom:3
        self.batch, self.depth = batch, depth
        nv, npub, nc = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().zkr_rollup_info(batch, depth, ctypes.byref(nv), ctypes.byref(npub), ctypes.byref(nc)))
        self.n_vars, self.n_public, self.n_constraints = nv.value, npub.value, nc.value

    def r1cs(self) -> bytes:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_rollup_r1cs(self.batch, self.depth, ctypes.byref(p), ctypes.byref(n)))
        return _take(p, n.value)

    def flatten_inputs(self, inputs):
        """The circuitInputs object of the reference (one entry per input signal of BatchProcessTx, arrays over the
        batch; batchprocesstx.test.ts builds it) -> the flat list in signal order."""
        flat = []

        def walk(v):
            if isinstance(v, (list, tuple)):
                for x in v:
                    walk(x)
            else:
                flat.append(int(v) % SNARK_FIELD_SIZE)
        for f in TX_INPUT_FIELDS:
            walk(inputs[f])
        if len(flat) != self.n_public - 1:
            raise ZkrError(-5, "circuit inputs have %d values, BatchProcessTx(%d, %d) takes %d" % (len(flat), self.batch, self.depth, self.n_public - 1))
        return flat

    def calculate_witness(self, inputs) -> bytes:
        flat = self.flatten_inputs(inputs) if isinstance(inputs, dict) else [int(v) for v in inputs]
        buf = b"".join(_le(v) for v in flat)
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_rollup_witness(self.batch, self.depth, buf, len(flat), ctypes.byref(p), ctypes.byref(n)))
        return _take(p, n.value)

    def public_signals(self, witness_bin: bytes):
        """witness.slice(1, nPubInputs + nOutputs + 1) (common.ts:18-21)."""
        return _ints(witness_bin[32:32 * (self.n_public + 1)])

    def witness_program_host(self, inputs):
        """The GPU builder's per-transaction program (csrc/rollup_witness.hpp) run on the host for one batch (test hook):
        (witness bytes, statement text of the first violation or None, its transaction)."""
        flat = self.flatten_inputs(inputs) if isinstance(inputs, dict) else [int(v) for v in inputs]
        buf = b"".join(_le(v) for v in flat)
        out = ctypes.create_string_buffer(self.n_vars * 32)
        stmt, tx = ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().zkr_rollup_witness_program_host(self.batch, self.depth, buf, len(flat), out, ctypes.byref(stmt), ctypes.byref(tx)))
        return out.raw, (lib().zkr_rollup_statement_text(stmt.value).decode() if stmt.value else None), tx.value

    def calculate_witness_batch_device(self, inputs_list, device=0):
        """calculateWitness for MANY rollup batches on the GPU (zkr_rollup_witness_batch_device: one thread per transaction):
        a uint8 torch tensor [len(inputs_list), nVars * 32] in HBM, row i = the bytes calculate_witness(inputs_list[i])
        returns, ready for ProvingKey.prove_batch_device([t[i].data_ptr() ...]).  Raises ZkrError(-7) naming the first batch,
        transaction and statement that fails."""
        import torch
        flats = [self.flatten_inputs(x) if isinstance(x, dict) else [int(v) for v in x] for x in inputs_list]
        for f in flats:
            if len(f) != self.n_public - 1:
                raise ZkrError(-5, "circuit inputs have %d values, BatchProcessTx(%d, %d) takes %d" % (len(f), self.batch, self.depth, self.n_public - 1))
        buf = b"".join(_le(v) for f in flats for v in f)
        out = torch.empty((len(flats), self.n_vars * 32), dtype=torch.uint8, device=torch.device("cuda", device))   # an allocation: nothing to wait for
        _check(lib().zkr_rollup_witness_batch_device(self.batch, self.depth, buf, self.n_public - 1, len(flats), out.data_ptr(), device))
        return out

    def calculate_witness_batch_from_device(self, inputs, stream=None):
        """calculate_witness_batch_device for inputs that are already in device memory (zkr_rollup_witness_batch_from_device):
        `inputs` = the uint8 tensor [n_batches, (n_public - 1) * 32] of Ledger.sequence.  Same kernels, same errors, same bytes."""
        import torch
        if inputs.dtype != torch.uint8 or inputs.dim() != 2 or inputs.shape[1] != (self.n_public - 1) * 32 or not inputs.is_cuda:
            raise ZkrError(-5, "circuit inputs must be a uint8 device tensor [n_batches, %d]" % ((self.n_public - 1) * 32))
        inputs = inputs.contiguous()
        device = inputs.device.index or 0
        out = torch.empty((inputs.shape[0], self.n_vars * 32), dtype=torch.uint8, device=inputs.device)
        _check(lib().zkr_rollup_witness_batch_from_device(self.batch, self.depth, inputs.data_ptr(), self.n_public - 1, inputs.shape[0], out.data_ptr(), device, stream))
        return out


class WithdrawCircuit:
    """Withdraw() (prover/circuits/withdraw.circom:4-25): public signals publicKey[0], publicKey[1], nullifier."""
    n_public = 3

    def r1cs(self) -> bytes:
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_withdraw_r1cs(ctypes.byref(p), ctypes.byref(n)))
        return _take(p, n.value)

    def calculate_witness(self, inputs) -> bytes:
        """inputs = {"privateKey": formatted key, "nullifier": ...} (withdraw.test.ts:22-25)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_withdraw_witness(_le(int(inputs["privateKey"])), _le(int(inputs["nullifier"]) % SNARK_FIELD_SIZE), ctypes.byref(p), ctypes.byref(n)))
        return _take(p, n.value)

    def public_signals(self, witness_bin: bytes):
        return _ints(witness_bin[32:128])

    @property
    def n_vars(self):
        return lib().zkr_withdraw_n_vars()

    def witness_program_host(self, inputs):
        """The GPU builder's per-witness program (csrc/wallet_program.hpp) run on the host (test hook): (witness bytes, None), or
        (None, the text of the first violated statement)."""
        out = ctypes.create_string_buffer(self.n_vars * 32)
        stmt = ctypes.c_uint32()
        _check(lib().zkr_withdraw_witness_program_host(_le(int(inputs["privateKey"])), _le(int(inputs["nullifier"])), out, ctypes.byref(stmt)))
        if stmt.value:
            return None, lib().zkr_withdraw_statement_text(stmt.value).decode()
        return out.raw, None

    def calculate_witness_batch_device(self, cases, device=0, stream=None):
        """calculateWitness for MANY withdrawals on the GPU (zkr_withdraw_witness_batch_device: one thread per witness): cases = a
        list of {"privateKey": formatted key, "nullifier": ...}.  A uint8 torch tensor [len(cases), nVars * 32] in HBM, row i =
        the bytes calculate_witness(cases[i]) returns, ready for ProvingKey.prove_batch_device([t[i].data_ptr() ...]).  The
        kernels run on `stream` (a raw stream handle; None: the default stream).  An input not below r is ZkrError(-5) -- the
        nullifier is NOT taken mod r here; a key past 253 bits ZkrError(-7) naming the first such witness and the statement."""
        import torch
        keys = b"".join(_le(int(x["privateKey"])) for x in cases)
        nuls = b"".join(_le(int(x["nullifier"])) for x in cases)
        out = torch.empty((len(cases), self.n_vars * 32), dtype=torch.uint8, device=torch.device("cuda", device))
        _check(lib().zkr_withdraw_witness_batch_device(keys, nuls, len(cases), out.data_ptr(), device, stream))
        return out


class BalanceTree:
    """operator/src/utils/merkletree.ts:14-83 as a full binary tree over the native hash: `depth` levels,
    2^depth leaves, empty leaf = zero value; `path(i)` = getUpdatePath(i).pathElements."""

    def __init__(self, depth, zero=0):
        self.depth = depth
        self.levels = [[zero] * (1 << depth)]
        z = zero
        for _ in range(depth):                       # an empty tree needs one hash per level
            z = hash_left_right(z, z)
            self.levels.append([z] * (len(self.levels[-1]) // 2))

    @classmethod
    def from_leaves(cls, depth, leaves, zero=0, device=0):
        """The tree over `leaves` (padded with the zero value) built on the GPU (zkr_balance_tree_build)."""
        t = cls.__new__(cls)
        t.depth = depth
        n = 1 << depth
        full = [int(v) for v in leaves] + [zero] * (n - len(leaves))
        out = ctypes.create_string_buffer(32 * (2 * n - 1))
        _check(lib().zkr_balance_tree_build(b"".join(_le(v) for v in full), depth, out, device))
        vals, t.levels, off = _ints(out.raw), [], 0
        for l in range(depth + 1):
            t.levels.append(vals[off:off + (n >> l)])
            off += n >> l
        return t

    @property
    def root(self):
        return self.levels[-1][0]

    def update(self, idx, leaf):
        self.levels[0][idx] = leaf
        for l in range(self.depth):
            idx >>= 1
            self.levels[l + 1][idx] = hash_left_right(self.levels[l][2 * idx], self.levels[l][2 * idx + 1])

    def path(self, idx):
        out = []
        for l in range(self.depth):
            out.append(self.levels[l][idx ^ 1])
            idx >>= 1
        return out


class RollupState:
    """The operator's side of a batch (the flow of operator/__tests__/operatorLogic.test.ts:100-222 and
    prover/__tests__/processtx.test.ts:24-130): accounts in a balance tree; `transfer` signs one transaction, applies
    it and returns its ProcessTx inputs; `batch_inputs` stacks them into the circuitInputs of BatchProcessTx."""

    def __init__(self, depth=6):
        self.tree = BalanceTree(depth)
        self.accounts = {}

    def deposit(self, index, pub, balance, nonce=0):
        self.accounts[index] = [int(pub[0]), int(pub[1]), int(balance), int(nonce)]
        self.tree.update(index, multi_hash(self.accounts[index]))       # hashBalanceTreeLeaf, helpers.ts:80-82

    def transfer(self, frm, to, amount, fee, priv):
        sa, ra, tree = self.accounts[frm], self.accounts[to], self.tree
        nonce = sa[3] + 1
        sig = sign(priv, [frm, to, amount, fee, nonce])                 # formatTx, helpers.ts:59-73
        inp = dict(balanceTreeRoot=tree.root, txData=[frm, to, amount, fee, nonce, sig["R8"][0], sig["R8"][1], sig["S"]],
                   txSenderPublicKey=sa[:2], txSenderBalance=sa[2], txSenderNonce=sa[3], txSenderPathElements=tree.path(frm),
                   txRecipientPublicKey=ra[:2], txRecipientBalance=ra[2], txRecipientNonce=ra[3], txRecipientPathElements=tree.path(to))
        sa[2] -= amount + fee
        sa[3] = nonce
        tree.update(frm, multi_hash(sa))
        inp["intermediateBalanceTreeRoot"] = tree.root
        inp["intermediateBalanceTreePathElements"] = tree.path(to)
        ra[2] += amount                                                 # the same record when frm == to (processtx.circom:141-159)
        tree.update(to, multi_hash(ra))
        return inp

    @staticmethod
    def batch_inputs(txs):
        return {f: [t[f] for t in txs] for f in TX_INPUT_FIELDS}
