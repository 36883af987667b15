// ledger_state.hpp -- the HOST side of keeping a ledger: the ZKRLEDG1 snapshot (header, tag, parser and check) and
// the bookkeeping of the checkpoint journal.  Plain C++ (no HIP): zkr_sequencer.hip uses it around its kernels,
// zkr_ledger_snapshot_check exposes the check to callers without a device, and ledger_state_selfcheck.cpp drives both under the
// sanitizers.  Stands in for the load / save of /root/reference/operator/src/utils/merkletree.ts:274-403, which trusts the root
// it stored; here the tag pins the header and the rebuilt root pins the records.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

namespace zkr {

enum : size_t { LEDGER_HEADER_BYTES = 128, LEDGER_RECORD_BYTES = 128 };

struct LedgerHeader {
  uint32_t depth = 0;
  uint64_t accounts = 0, applied = 0, batches = 0;
  uint8_t root[32] = {0};
};

// The 128 header bytes of a snapshot: magic, depth, counters, root and the tag over all of them.  0, or -1 when the hash refuses.
int ledger_header_write(const LedgerHeader &h, uint8_t out[LEDGER_HEADER_BYTES]);
// The whole check of include/zkr.h zkr_ledger_snapshot_check.  0 and *h filled in, or -1 with `why` naming the first failure.
int ledger_snapshot_parse(const uint8_t *blob, size_t len, LedgerHeader *h, char *why, size_t why_len);

// ---- the checkpoint journal's host side.  Every storing call made while a checkpoint is open leaves one JournalCall: where its
// (node offset, old value) pairs lie in the device journal, the records it overwrote and the counters before it.  Checkpoints
// are markers between calls.
struct JournalCall {
  size_t node_begin = 0, node_count = 0;  // entries [node_begin, node_begin + node_count) of the device journal
  size_t accounts_before = 0;
  uint64_t applied_before = 0, batches_before = 0;
  std::vector<uint32_t> rec_idx;  // overwritten records that existed before the call ...
  std::vector<uint8_t> rec_old;   // ... and what they held, 128 B each
  // with a book open: the nullifier count and the fee counter before the call
  bool has_book = false;
  size_t nullifiers_before = 0;
  uint64_t fees_before[4] = {0, 0, 0, 0};
};
struct JournalMarker {
  uint64_t id;
  size_t calls;  // calls journalled when the checkpoint was taken
};
struct LedgerJournal {
  std::vector<JournalCall> calls;
  std::vector<JournalMarker> markers;  // oldest first; ids ascend
  uint64_t next_id = 1;

  bool open() const { return !markers.empty(); }
  size_t nodes() const { return calls.empty() ? 0 : calls.back().node_begin + calls.back().node_count; }
  uint64_t checkpoint() {
    markers.push_back(JournalMarker{next_id, calls.size()});
    return next_id++;
  }
  int find(uint64_t id) const {  // position among the open markers, or -1
    for (size_t i = 0; i < markers.size(); i++)
      if (markers[i].id == id) return (int)i;
    return -1;
  }
  // release: the marker goes, the state stays; with the last marker the journal is emptied.  false: no such checkpoint
  bool release(uint64_t id) {
    const int at = find(id);
    if (at < 0) return false;
    markers.erase(markers.begin() + at);
    if (markers.empty()) calls.clear();
    return true;
  }
  // rollback, step 1: how many calls stay (the caller undoes calls.size() - 1 down to this, in that order); -1: no such checkpoint
  long rollback_keep(uint64_t id) const {
    const int at = find(id);
    return at < 0 ? -1 : (long)markers[at].calls;
  }
  // rollback, step 2, after the undo: the calls and every checkpoint taken after `id` go, `id` stays open
  void rollback_done(uint64_t id) {
    const int at = find(id);
    if (at < 0) return;
    calls.resize(markers[at].calls);
    markers.resize((size_t)at + 1);
  }
  // One call's host part: the records of `idx` as they stand in `records` (accounts x 128 B) before the call moves them.
  JournalCall record_call(const uint32_t *idx, size_t n, const std::vector<uint8_t> &records, size_t accounts, uint64_t applied, uint64_t batches,
                          size_t node_count) const {
    JournalCall c;
    c.node_begin = nodes(), c.node_count = node_count;
    c.accounts_before = accounts, c.applied_before = applied, c.batches_before = batches;
    for (size_t u = 0; u < n; u++) {
      if (idx[u] >= accounts) continue;  // an account the call inserts: it disappears with the account count
      c.rec_idx.push_back(idx[u]);
      c.rec_old.insert(c.rec_old.end(), records.begin() + (size_t)idx[u] * LEDGER_RECORD_BYTES, records.begin() + ((size_t)idx[u] + 1) * LEDGER_RECORD_BYTES);
    }
    return c;
  }
  // The host part of undoing call `c`: records, account count and counters as they stood before it.
  static void undo_host(const JournalCall &c, std::vector<uint8_t> &records, size_t &accounts, uint64_t &applied, uint64_t &batches) {
    records.resize(c.accounts_before * LEDGER_RECORD_BYTES);
    for (size_t i = 0; i < c.rec_idx.size(); i++)  // an index met twice holds the same bytes twice: both are from before the call
      memcpy(records.data() + (size_t)c.rec_idx[i] * LEDGER_RECORD_BYTES, c.rec_old.data() + i * LEDGER_RECORD_BYTES, LEDGER_RECORD_BYTES);
    accounts = c.accounts_before, applied = c.applied_before, batches = c.batches_before;
  }
};

}  // namespace zkr
