"""The model the sequencer tests hold zkr_ledger_sequence to (tests/test_sequencer_cpu.py, tests/test_gpu_sequencer.py): the
rule list of include/zkr.h applied one transaction at a time in Python over oracle/rollup.py (verify, Tree, leaf_hash and the
state transition of process_tx_inputs).  Not a test module."""
import copy
import functools

import rollup as o

P250 = 1 << 250
NOT_REACHED = 255


def sig_ok_oracle(row, pub):
    """Rule 10: the oracle's `verify` over multiHash([from, to, amount, fee, nonce]), and the circuit's refusal of a key whose
    order divides 8 (eddsa.circom's patched verifier: 4A must not have x = 0)."""
    if any(v >= o.R for v in list(row[5:8]) + list(pub)):
        return False
    if not o.verify(row[:5], (row[5], row[6], row[7]), tuple(pub)):
        return False
    return o.bj_mul(tuple(pub), 4)[0] != 0


def status_of(accounts, row, sig_ok):
    """The first rule of the list `row` breaks against `accounts` ({index: [pubX, pubY, balance, nonce]}, indices 0..n-1), 0 = none."""
    frm, to, amount, fee, nonce = row[:5]
    if frm not in accounts:
        return 1
    if to not in accounts:
        return 2
    if any(v >= o.R for v in row) or amount >= P250 or fee >= P250 or nonce >= P250:
        return 3
    if amount == 0:
        return 4
    if fee == 0:
        return 5
    s, r = accounts[frm], accounts[to]
    if not s[2] > amount + fee:
        return 6
    if not fee >= (amount // 1000) * 3:
        return 7
    if nonce != s[3] + 1:
        return 8
    new_recipient = s[2] - fee if frm == to else r[2] + amount
    if new_recipient >= P250:
        return 9
    if not sig_ok(row, s[:2]):
        return 10
    return 0


def apply_tx(tree, accounts, row):
    """oracle/rollup.py process_tx_inputs for a transaction that arrives signed: the same reads and writes in the same order."""
    frm, to, amount, fee, nonce = row[:5]
    sa, ra = accounts[frm], accounts[to]
    inp = dict(balanceTreeRoot=tree.root, txData=list(row),
               txSenderPublicKey=sa[:2], txSenderBalance=sa[2], txSenderNonce=sa[3], txSenderPathElements=tree.path(frm),
               txRecipientPublicKey=ra[:2], txRecipientBalance=ra[2], txRecipientNonce=ra[3], txRecipientPathElements=tree.path(to))
    sa[2] -= amount + fee
    sa[3] = nonce
    tree.update(frm, o.leaf_hash(sa[:2], sa[2], sa[3]))
    inp["intermediateBalanceTreeRoot"] = tree.root
    inp["intermediateBalanceTreePathElements"] = tree.path(to)
    ra = accounts[to]
    ra[2] += amount
    tree.update(to, o.leaf_hash(ra[:2], ra[2], ra[3]))
    inp["newBalanceTreeRoot"] = tree.root
    return inp


class Model:
    """Accounts and (optionally) the balance tree, as the ledger keeps them."""

    def __init__(self, depth, with_tree=True):
        self.depth = depth
        self.accounts = {}
        self.tree = o.Tree(depth) if with_tree else None

    def deposit(self, index, pub, balance, nonce=0):
        assert index <= len(self.accounts)
        self.accounts[index] = [int(pub[0]), int(pub[1]), int(balance), int(nonce)]
        if self.tree:
            self.tree.update(index, o.leaf_hash(pub, balance, nonce))

    def records(self):
        return [list(self.accounts[i]) for i in range(len(self.accounts))]

    def sequence(self, rows, batch, sig_ok=sig_ok_oracle):
        """-> (statuses, inputs per batch as the flat signal list WITHOUT the output, consumed, leaf index per update).  The state
        moves to the one after the last applied transaction."""
        trial = copy.deepcopy(self.accounts)
        status, accepted = [], []
        for t, row in enumerate(rows):
            st = status_of(trial, row, sig_ok)
            status.append(st)
            if st == 0:
                accepted.append(t)
                frm, to, amount, fee, nonce = row[:5]
                trial[frm][2] -= amount + fee
                trial[frm][3] = nonce
                trial[to][2] += amount
        T = len(accepted) - len(accepted) % batch
        consumed = accepted[T - 1] + 1 if T else 0
        status = status[:consumed] + [NOT_REACHED] * (len(rows) - consumed)
        applied, idx = [], []
        for t in accepted[:T]:
            idx += [rows[t][0], rows[t][1]]
            if self.tree:
                applied.append(apply_tx(self.tree, self.accounts, rows[t]))
            else:
                frm, to, amount, fee, nonce = rows[t][:5]
                self.accounts[frm][2] -= amount + fee
                self.accounts[frm][3] = nonce
                self.accounts[to][2] += amount
        inputs = [o.batch_public_signals(applied[b:b + batch])[1:] for b in range(0, len(applied), batch)]
        return status, inputs, consumed, idx


def brute_tables(depth, idx):
    """The three look-up tables of include/zkr.h (zkr_sequence_plan_host) by exhaustive search over the earlier updates."""
    U = len(idx)

    def latest(l, node, before):
        return max([u for u in range(before) if idx[u] >> l == node], default=-1)
    t0 = [[latest(l, (idx[u] >> l) ^ 1, u) for u in range(U)] for l in range(depth)]
    t1 = [[latest(l, (idx[u + 1] >> l) ^ 1, u) if u % 2 == 0 else -1 for u in range(U)] for l in range(depth)]
    t2 = [[0 if any(idx[v] >> l == idx[u] >> l for v in range(u + 1, U)) else 1 for u in range(U)] for l in range(depth)]
    return [t0, t1, t2]


# ---- signed fixtures (zkr_hip.rollup.sign; host code, no device)
@functools.lru_cache(maxsize=None)
def keypair(i):
    from zkr_hip import rollup as n
    priv = 0x1000 + 7 * i
    return priv, n.gen_public_key(priv)


def signed_row(frm, to, amount, fee, nonce, signer=None):
    from zkr_hip import rollup as n
    priv, _ = keypair(frm if signer is None else signer)
    return n.tx_row(frm, to, amount, fee, nonce, n.sign(priv, [frm, to, amount, fee, nonce]))


def le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)
