// sequencer_plan.hpp -- the HOST pass of the transaction sequencer (zkr_ledger_sequence, step b of DESIGN.md 9f): the operator's
// rules of /root/reference/operator/src/routes/send.ts:72-135 applied to a queue in order, the balance and nonce arithmetic, and
// the look-up tables that let the device rebuild every intermediate tree level by level.  Plain C++ (no HIP): zkr_sequencer.hip
// runs it between the signature kernel and the hashes, zkr_sequence_plan_host exposes it to the CPU suite, and
// sequencer_selfcheck.cpp drives it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

namespace zkr {

struct Int256 {  // little-endian words; the 32 B standard form of a field element read as an integer
  uint64_t w[4];
};
inline Int256 int256_load(const uint8_t *p) { Int256 a; memcpy(a.w, p, 32); return a; }
inline void int256_store(uint8_t *p, const Int256 &a) { memcpy(p, a.w, 32); }
inline Int256 int256_small(uint64_t v) { return Int256{{v, 0, 0, 0}}; }
inline int int256_cmp(const Int256 &a, const Int256 &b) {
  for (int i = 3; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
  return 0;
}
inline bool int256_is_zero(const Int256 &a) { return !(a.w[0] | a.w[1] | a.w[2] | a.w[3]); }
inline Int256 int256_add(const Int256 &a, const Int256 &b) {  // mod 2^256; the callers' operands are below 2^251
  Int256 r;
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (unsigned __int128)a.w[i] + b.w[i];
    r.w[i] = (uint64_t)c;
    c >>= 64;
  }
  return r;
}
inline Int256 int256_sub(const Int256 &a, const Int256 &b) {  // a >= b
  Int256 r;
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    unsigned __int128 d = (unsigned __int128)a.w[i] - b.w[i] - br;
    r.w[i] = (uint64_t)d;
    br = (uint64_t)(d >> 64) & 1;
  }
  return r;
}
inline Int256 int256_div_small(const Int256 &a, uint64_t d) {
  Int256 q;
  unsigned __int128 rem = 0;
  for (int i = 3; i >= 0; i--) {
    unsigned __int128 cur = (rem << 64) | a.w[i];
    q.w[i] = (uint64_t)(cur / d);
    rem = cur % d;
  }
  return q;
}
inline Int256 int256_mul_small(const Int256 &a, uint64_t m) {  // mod 2^256
  Int256 r;
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (unsigned __int128)a.w[i] * m;
    r.w[i] = (uint64_t)c;
    c >>= 64;
  }
  return r;
}
inline bool int256_below_2_250(const Int256 &a) { return (a.w[3] >> 58) == 0; }
bool int256_below_r(const Int256 &a);  // the scalar field's modulus (field.hpp FrParams::P)

struct SeqRecord {  // pubX pubY balance nonce
  Int256 f[4];
};

// status codes of zkr_ledger_sequence (include/zkr.h): 0 accepted, 1..10 the first broken rule, 255 not reached
enum : uint8_t { SEQ_NOT_REACHED = 255 };

struct SeqPlan {
  std::vector<uint8_t> status;      // n_txs
  size_t consumed = 0;              // queue position just behind the last applied transaction
  size_t applied = 0;               // T
  std::vector<uint32_t> pos;        // T: queue position of applied transaction k
  std::vector<uint32_t> idx;        // 2T: the leaf update u writes (u = 2k the sender, 2k + 1 the recipient)
  std::vector<SeqRecord> old_rec;   // 2T: the sender's / recipient's record BEFORE transaction k (the circuit's inputs)
  std::vector<SeqRecord> new_rec;   // 2T: the record update u leaves in its leaf
  std::vector<int32_t> prev;        // 3 x depth x 2T, see seq_tables
};

// The look-up tables of a list of leaf updates, [3][depth][U] (U = idx.size()):
//   table 0, [l][u]   the latest update u' < u under the SIBLING of node idx[u] >> l at level l, or -1: the tree's stored node
//   table 1, [l][2k]  the same query for node query1[k] >> l, asked before update 2k (the recipient's path before its
//                     transaction); odd positions and a null query1 leave -1
//   table 2, [l][u]   1 when no later update touches node idx[u] >> l of level l (u holds the node's last version), else 0
// n_leaves bounds every index (checked by the callers).
void seq_tables(unsigned depth, const std::vector<uint32_t> &idx, const uint32_t *query1, size_t n_leaves, int32_t *out);

// The pass.  records: n_accounts x 128 B; txs: n_txs x 256 B; sig_verdicts: n_txs bytes, non-zero = rule 10 holds.
// Returns 0, or -1 with *why set for arguments that cannot be sequenced (a record that is no field element, ...).
int seq_plan(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *txs, size_t n_txs, const uint8_t *sig_verdicts,
             uint32_t batch, SeqPlan &out, const char **why);

// The pass of a REPLAY (zkr_ledger_replay): the state update of RollUp.sol:118-158 for a run of published batches,
// from their txData alone.  This is the contract's arithmetic, not the operator's policy: of the sequencer's rules only 1, 2, 3
// and 9 remain, and a sender needs balance >= amount + fee.  Positive amount and fee, the strict balance, the fee floor and
// nonce + 1 (rules 4-8) are NOT applied -- the contract applies whatever was proved, and what the circuit enforces is the proof's
// matter; a follower has to track the contract.  The sender's leaf moves first (balance - amount - fee, nonce := the
// transaction's), then the recipient's (balance + amount), from == to included (processtx.circom:141-159).
// publics: n_batches x n_public x 32 B, n_public = 1 + batch * (18 + 3 * depth), circom's order; only the < r check reads
// anything but the txData rows (signal 1 + batch + 8k + j of a batch).
// Batches are planned in order until one cannot be applied; *planned is its index (n_batches: none), *where the offending
// signal: the lowest signal not below r, else for the first transaction it holds for: `from` / `to` no account; amount, fee or
// nonce not below 2^250; and, at the transaction's amount signal, a sender balance below amount + fee or a recipient balance
// that would reach 2^250.  out holds the planned batches' updates as seq_plan leaves them (pos[k] = k, consumed = applied =
// *planned * batch, status empty), which is exactly what keeps the arithmetic and the kernels' indices in range without a proof.
int replay_plan(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *publics, size_t n_batches, uint32_t batch,
                SeqPlan &out, size_t *planned, uint32_t *where, const char **why);

}  // namespace zkr
