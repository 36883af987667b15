// ledger_state.cpp -- the ZKRLEDG1 snapshot of a ledger on the host (ledger_state.hpp): header and tag, the parser
// and zkr_ledger_snapshot_check.  Nothing here touches a device; zkr_ledger_restore (zkr_sequencer.hip) runs this check before
// it looks for one.
#include "ledger_state.hpp"

#include <stdio.h>

#include "../../include/zkr.h"
#include "sequencer_plan.hpp"

namespace zkr {
void set_error(const char *fmt, ...);

static const char LEDGER_MAGIC[9] = "ZKRLEDG1";

static void put_u32(uint8_t *p, uint32_t v) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static void put_u64(uint8_t *p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static uint32_t get_u32(const uint8_t *p) { uint32_t v = 0; for (int i = 0; i < 4; i++) v |= (uint32_t)p[i] << (8 * i); return v; }
static uint64_t get_u64(const uint8_t *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

// tag = multiHash(depth, accounts, applied, batches, root)
static int ledger_tag(const LedgerHeader &h, uint8_t tag[32]) {
  uint8_t in[5 * 32] = {0};
  put_u64(in, h.depth), put_u64(in + 32, h.accounts), put_u64(in + 64, h.applied), put_u64(in + 96, h.batches);
  memcpy(in + 128, h.root, 32);
  return zkr_mimcsponge_multihash(in, 5, tag) == ZKR_OK ? 0 : -1;
}

int ledger_header_write(const LedgerHeader &h, uint8_t out[LEDGER_HEADER_BYTES]) {
  memset(out, 0, LEDGER_HEADER_BYTES);
  memcpy(out, LEDGER_MAGIC, 8);
  put_u32(out + 8, h.depth);
  put_u64(out + 16, h.accounts), put_u64(out + 24, h.applied), put_u64(out + 32, h.batches);
  memcpy(out + 64, h.root, 32);
  return ledger_tag(h, out + 96);
}

int ledger_snapshot_parse(const uint8_t *blob, size_t len, LedgerHeader *h, char *why, size_t why_len) {
#define refuse(...) (snprintf(why, why_len, __VA_ARGS__), -1)
  if (len < LEDGER_HEADER_BYTES) return refuse("ledger snapshot: length %zu is shorter than the %zu header bytes", len, (size_t)LEDGER_HEADER_BYTES);
  if (memcmp(blob, LEDGER_MAGIC, 8)) return refuse("ledger snapshot: wrong magic (not ZKRLEDG1)");
  if (get_u32(blob + 12)) return refuse("ledger snapshot: reserved word at offset 12 is not zero");
  for (size_t i = 40; i < 64; i++)
    if (blob[i]) return refuse("ledger snapshot: reserved byte at offset %zu is not zero", i);
  LedgerHeader hd;
  hd.depth = get_u32(blob + 8);
  hd.accounts = get_u64(blob + 16), hd.applied = get_u64(blob + 24), hd.batches = get_u64(blob + 32);
  memcpy(hd.root, blob + 64, 32);
  if (hd.depth < 1 || hd.depth > 24) return refuse("ledger snapshot: depth %u out of range (1..24)", hd.depth);
  if (hd.accounts > ((uint64_t)1 << hd.depth)) return refuse("ledger snapshot: %llu accounts do not fit a tree of depth %u", (unsigned long long)hd.accounts, hd.depth);
  const size_t want = LEDGER_HEADER_BYTES + LEDGER_RECORD_BYTES * (size_t)hd.accounts;
  if (len != want) return refuse("ledger snapshot: length %zu, but %llu accounts make %zu bytes", len, (unsigned long long)hd.accounts, want);
  uint8_t tag[32];
  if (ledger_tag(hd, tag)) return refuse("ledger snapshot: the tag could not be computed");
  if (memcmp(tag, blob + 96, 32)) return refuse("ledger snapshot: the tag does not match the header (depth, counters or root were changed)");
  if (!int256_below_r(int256_load(hd.root))) return refuse("ledger snapshot: the root is not below r");
  for (size_t i = 0; i < (size_t)hd.accounts; i++)
    for (int j = 0; j < 4; j++) {
      const Int256 v = int256_load(blob + LEDGER_HEADER_BYTES + i * LEDGER_RECORD_BYTES + 32 * j);
      if (!int256_below_r(v)) return refuse("ledger snapshot: record %zu element %d is not below r", i, j);
      if (j >= 2 && !int256_below_2_250(v)) return refuse("ledger snapshot: record %zu %s does not fit the circuit's 250 bits (not below 2^250)", i, j == 2 ? "balance" : "nonce");
    }
#undef refuse
  *h = hd;
  return 0;
}

}  // namespace zkr

using namespace zkr;

extern "C" int zkr_ledger_snapshot_check(const void *blob, size_t len, uint64_t info[4], int *valid) {
  if (valid) *valid = 0;
  if (!blob || !info || !valid) { set_error("null argument"); return ZKR_ERR_ARG; }
  LedgerHeader h;
  char why[200];
  if (ledger_snapshot_parse((const uint8_t *)blob, len, &h, why, sizeof why)) { set_error("%s", why); return ZKR_OK; }
  info[0] = h.depth, info[1] = h.accounts, info[2] = h.applied, info[3] = h.batches;
  *valid = 1;
  return ZKR_OK;
}
