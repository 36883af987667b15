// ledger_internal.hpp -- what the ledger's two HIP units share: zkr_sequencer.hip (queue to batches, replay, keeping the state) and
// zkr_book.hip (the contract's key-addressed side).  The ledger handle, its arena, the view a storing call leaves in
// device memory, and the two steps of the one storing path -- stage_updates, store_updates -- which stay where their kernels are,
// in zkr_sequencer.hip (no relocatable device code in this build: a kernel is launched from the unit that holds it).
#pragma once
#include <stdlib.h>
#include <chrono>
#include <mutex>
#include <vector>
#include "zkr_internal.hpp"
#include "sequencer_plan.hpp"
#include "ledger_state.hpp"

namespace zkr {

__host__ __device__ static inline size_t seq_level_offset(uint32_t depth, uint32_t l) {  // leaves first, root last (zkr_balance_tree_build's order)
  return ((size_t)2 << depth) - ((size_t)2 << (depth - l));
}
struct SeqView {  // what one call left in device memory; U = 2T updates
  const Fr *txs;        // T x 8, the applied transactions
  const Fr *old_rec;    // U x 4
  const Fr *val;        // (depth + 1) rows of `stride`, the first U of each in use
  const uint32_t *idx;  // U
  const int32_t *prev;  // 3 x depth x U (sequencer_plan.hpp seq_tables)
  const Fr *tree;       // the ledger's stored tree, before this call
  size_t U, stride;     // stride > U: a prefix of the updates that were hashed (a replay that stops at a refused batch)
  uint32_t depth, batch;
};

static inline unsigned blocks(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

struct DevArena {  // one allocation per ledger, only ever grown; cut into aligned pieces per call
  Dev<char> p;
  size_t cap = 0, at = 0;
  int reserve(size_t bytes) {
    at = 0;
    if (bytes <= cap) return ZKR_OK;
    cap = 0;
    if (int rc = p.alloc(bytes + bytes / 2)) return rc;  // the old block goes first: a call keeps nothing in the arena
    cap = bytes + bytes / 2;
    return ZKR_OK;
  }
  static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  template <class T> T *take(size_t count) {
    T *r = reinterpret_cast<T *>(p + at);
    at += padded(count * sizeof(T));
    return r;
  }
};

// The book of a ledger (zkr_book.hip): the contract's key-addressed state beside the tree.  Everything a d_ pointer
// names lives on the ledger's device and goes with the book, which goes with the ledger.
struct LedgerBook {
  // key table: d_keyhash[i] = hashPair(pubX, pubY) of record i; d_keytab holds index + 1 in 2^(depth + 1) slots, 0 = empty
  Dev<Fr> d_keyhash;
  Dev<uint32_t> d_keytab;
  bool keys_stale = true;
  uint64_t distinct = 0, rebuilds = 0;
  // nullifier set: d_null[0 .. null_count) in acceptance order; d_nulltab holds position + 1 in null_cap slots
  Dev<Fr> d_null;
  Dev<uint32_t> d_nulltab;
  size_t null_count = 0, null_room = 0, null_cap = 0;  // room: entries d_null has memory for
  bool null_stale = false;
  uint64_t salt = 0;
  Int256 fees = {{0, 0, 0, 0}};  // accuredFees (RollUp.sol:139)
};
}  // namespace zkr

struct zkr_ledger {
  unsigned depth = 0;
  int device = 0;
  size_t accounts = 0;
  uint64_t applied = 0, batches = 0;
  std::vector<uint8_t> records;  // accounts x 128 B
  zkr::Dev<zkr::Fr> d_tree;      // (2^(depth + 1) - 1) nodes, standard form, leaves first
  zkr::DevArena arena;
  double stage_ms[5] = {0, 0, 0, 0, 0};
  mutable std::mutex mu;
  // keeping the ledger
  std::vector<uint8_t> empty;    // (depth + 1) x 32 B: the value of an empty subtree per level
  zkr::LedgerJournal journal;    // checkpoints and what every storing call under them overwrote, host part
  zkr::Dev<uint32_t> d_joff;     // the journal's device part: node offsets ...
  zkr::Dev<zkr::Fr> d_jold;      // ... and old values, jcap entries each, the first journal.nodes() in use
  zkr::Dev<uint32_t> d_jcount;
  size_t jcap = 0;
  // the contract's side: null until zkr_ledger_book_open
  zkr::LedgerBook *book = nullptr;
  ~zkr_ledger() { delete book; }
};

namespace zkr {
struct StageClock {  // wall time per stage, only when ZKR_SEQUENCER_STAGES is set: every mark waits for the stream
  bool on;
  hipStream_t s;
  std::chrono::steady_clock::time_point t0;
  StageClock(hipStream_t stream) : on(getenv("ZKR_SEQUENCER_STAGES") != nullptr), s(stream), t0(std::chrono::steady_clock::now()) {}
  void mark(double &slot) {
    if (!on) return;
    hipStreamSynchronize(s);
    const auto t1 = std::chrono::steady_clock::now();
    slot = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

// ---- the storing path (zkr_sequencer.hip), under the ledger's lock: reserve the arena, stage_updates, what the caller derives from
// the hashes, store_updates, the caller's counters.  "On an error return the ledger is unchanged" is argued in these two steps:
// nothing before store_updates' first synchronise writes the tree, the journal moves after the store, the records move last.
struct UpdateList {  // U leaf updates on the host
  size_t U;
  const uint32_t *idx;               // U leaf indices
  const uint8_t *new_rec, *old_rec;  // U x 128 B each; old_rec is null where nothing is derived from it (a deposit)
  const int32_t *prev;               // 3 x depth x U (seq_tables)
};
struct StagedUpdates {  // the same list in the arena, hashed: val[l][u] for l <= depth
  Fr *d_old, *d_new, *d_val;
  uint32_t *d_idx;
  int32_t *d_prev;
  size_t U;
  // the view over the first `stored` updates (fewer than U only for a replay that stops early); val keeps the hashed list's rows
  SeqView view(const zkr_ledger *l, const Fr *txs, uint32_t batch, size_t stored) const {
    return SeqView{txs, d_old, d_val, d_idx, d_prev, l->d_tree, stored, U, l->depth, batch};
  }
};
size_t update_arena_bytes(size_t U_max, unsigned depth, bool with_old);  // what stage_updates cuts; a caller's reserve adds its own
// Bounds idx[u] < accounts and, with check_tables, -1 <= prev[l][u] < u (a plan's tables; ledger_apply_updates computes its own and
// never scanned them: profiles/ledger_refactor.md), cuts the arena, uploads, hashes leaves and levels (stage slots 2, 3).
int stage_updates(zkr_ledger *l, const UpdateList &in, size_t accounts, bool check_tables, hipStream_t s, StageClock &clk, double *ms, StagedUpdates *out);
// Synchronises, journals when a checkpoint is open, stores the last versions under v, synchronises, appends the journal's call,
// marks `slot` (stage slot 4) and copies the records into l->records, which has room for every index.  last = the stored list's
// table 2 on the host, idx and new_rec its leaf indices and records.  Counters stay with the caller.
int store_updates(zkr_ledger *l, const SeqView &v, const int32_t *last, const uint32_t *idx, const uint8_t *new_rec, hipStream_t s, StageClock &clk, double &slot);
// zkr_ledger_deposit behind its argument checks, and how the book applies its update lists; `accounts` = the count the list leaves
int ledger_apply_updates(zkr_ledger *l, const uint32_t *indices, const uint8_t *records, size_t n, size_t accounts);
}  // namespace zkr
