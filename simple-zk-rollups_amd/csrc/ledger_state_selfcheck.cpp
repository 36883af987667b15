// ledger_state_selfcheck.cpp -- a stand-alone program over the host side of keeping a ledger (ledger_state.cpp / .hpp: the
// ZKRLEDG1 snapshot's header, parser and check, and the checkpoint journal's bookkeeping), meant for a sanitizer build
// (`make ledger-asan`: AddressSanitizer + UBSan on this file, ledger_state.cpp, sequencer_plan.cpp and rollup.cpp, which has the
// tag's hash; no Python and no HIP in the process).  It feeds the parser well-formed blobs and the malformed ones of
// tests/test_ledger_state_cpu.py, each in an allocation of exactly its length, and plays nested checkpoints, rollbacks and
// releases over a model of the records.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "ledger_state.hpp"

extern "C" int zkr_ledger_snapshot_check(const void *blob, size_t len, uint64_t info[4], int *valid);
static char last_error[512];
namespace zkr {
void set_error(const char *fmt, ...) {  // the library's lives beside its HIP code
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof last_error, fmt, ap);
  va_end(ap);
}
bool rollup_witness_fast_host(uint32_t, uint32_t, const uint8_t *, uint8_t *) { return false; }  // rollup.cpp's witness shortcut lives in rollup_gpu.hip; unused here
}  // namespace zkr
using namespace zkr;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fails++; fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #x, last_error); } } while (0)

static uint64_t rng_state = 0x5A4B0009;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static void put(uint8_t *p, uint64_t v) {
  memset(p, 0, 32);
  memcpy(p, &v, 8);
}
static const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};  // r

static std::vector<uint8_t> snapshot(uint32_t depth, uint64_t accounts, uint64_t applied, uint64_t batches) {
  std::vector<uint8_t> b(LEDGER_HEADER_BYTES + accounts * LEDGER_RECORD_BYTES);
  LedgerHeader h;
  h.depth = depth, h.accounts = accounts, h.applied = applied, h.batches = batches;
  put(h.root, rnd() >> 8);  // the parser does not rebuild the tree: any element below r
  CHECK(ledger_header_write(h, b.data()) == 0);
  for (uint64_t i = 0; i < accounts; i++) {
    uint8_t *r = &b[LEDGER_HEADER_BYTES + i * LEDGER_RECORD_BYTES];
    put(r, rnd()), put(r + 32, rnd()), put(r + 64, rnd() % 100000), put(r + 96, rnd() % 50);
  }
  return b;
}
// the check over a copy that is exactly `len` bytes long, so that a read past the end is an error the sanitizer sees
static bool refused(const std::vector<uint8_t> &blob, const char *word) {
  std::vector<uint8_t> exact(blob);
  exact.shrink_to_fit();
  uint64_t info[4] = {7, 7, 7, 7};
  int valid = 7;
  last_error[0] = 0;
  const int rc = zkr_ledger_snapshot_check(exact.data(), exact.size(), info, &valid);
  return rc == 0 && valid == 0 && info[0] == 7 && strstr(last_error, word) != nullptr;
}

static void parser() {
  for (uint32_t depth = 1; depth <= 24; depth++) {
    const uint64_t cap = (uint64_t)1 << (depth > 7 ? 7 : depth);
    for (uint64_t accounts : {(uint64_t)0, (uint64_t)1, cap - 1, cap}) {
      std::vector<uint8_t> b = snapshot(depth, accounts, 12 + depth, 6);
      uint64_t info[4];
      int valid = 0;
      CHECK(zkr_ledger_snapshot_check(b.data(), b.size(), info, &valid) == 0 && valid == 1);
      CHECK(info[0] == depth && info[1] == accounts && info[2] == 12 + depth && info[3] == 6);
      LedgerHeader h;
      char why[64];  // a short message buffer: the parser's lines are longer than this
      std::vector<uint8_t> cut(b.begin(), b.end() - (accounts ? 1 : 0));
      CHECK(ledger_snapshot_parse(cut.data(), cut.size(), &h, why, sizeof why) == (accounts ? -1 : 0));
    }
  }
  const std::vector<uint8_t> good = snapshot(3, 5, 12, 6);
  std::vector<uint8_t> b;
  b = good, b[0] ^= 1;
  CHECK(refused(b, "magic"));
  b = good, b[13] = 1;
  CHECK(refused(b, "reserved"));
  b = good, b[63] = 0x80;
  CHECK(refused(b, "reserved"));
  b = good, b.pop_back();
  CHECK(refused(b, "length"));
  b = good, b.push_back(0);
  CHECK(refused(b, "length"));
  b.assign(good.begin(), good.begin() + 127);
  CHECK(refused(b, "length"));
  b.clear();
  b.push_back(0);
  CHECK(refused(b, "length"));
  b = good, b[8] = 0;
  CHECK(refused(b, "depth"));
  b = good, b[8] = 25;
  CHECK(refused(b, "depth"));
  b = good, b[16] = 9;  // 2^3 + 1 accounts
  CHECK(refused(b, "accounts"));
  b = good, memset(&b[16], 0xFF, 8);  // a count whose length would wrap
  CHECK(refused(b, "accounts"));
  b = good, b[96] ^= 1;
  CHECK(refused(b, "tag"));
  b = good, b[24] ^= 1;  // `applied` changed under the old tag
  CHECK(refused(b, "tag"));
  b = good, b[64] ^= 1;  // the root
  CHECK(refused(b, "tag"));
  b = good, memcpy(&b[128 + 2 * 128 + 32], R_LE, 32);  // pubY of record 2 = r
  CHECK(refused(b, "below r"));
  b = good, memset(&b[128 + 4 * 128 + 64], 0, 32), b[128 + 4 * 128 + 64 + 31] = 0x04;  // a balance of 2^250
  CHECK(refused(b, "2^250"));
  b = good, memset(&b[128 + 96], 0, 32), b[128 + 96 + 31] = 0x04;  // a nonce of 2^250
  CHECK(refused(b, "2^250"));
  uint64_t info[4];
  int valid = 5;
  CHECK(zkr_ledger_snapshot_check(nullptr, 128, info, &valid) == -5 && valid == 0);
  CHECK(zkr_ledger_snapshot_check(good.data(), good.size(), nullptr, &valid) == -5);
  CHECK(zkr_ledger_snapshot_check(good.data(), good.size(), info, nullptr) == -5);
}

// ---- the journal: random storing calls, checkpoints, rollbacks and releases against saved copies of the state
struct State {
  std::vector<uint8_t> records;
  size_t accounts = 0;
  uint64_t applied = 0, batches = 0;
  bool operator==(const State &o) const { return records == o.records && accounts == o.accounts && applied == o.applied && batches == o.batches; }
};
static void storing_call(State &s, LedgerJournal &j, size_t cap) {
  const size_t n = 1 + rnd() % 6;
  std::vector<uint32_t> idx;
  size_t accounts = s.accounts;
  for (size_t i = 0; i < n; i++) {
    uint32_t at = (uint32_t)(rnd() % (accounts + 1));
    if (at == accounts && accounts == cap) at = 0;
    if (at == accounts) accounts++;
    idx.push_back(at);
  }
  const size_t nodes = 1 + rnd() % 9;
  if (j.open()) j.calls.push_back(j.record_call(idx.data(), n, s.records, s.accounts, s.applied, s.batches, nodes));
  s.records.resize(accounts * LEDGER_RECORD_BYTES);
  for (uint32_t at : idx) put(&s.records[(size_t)at * LEDGER_RECORD_BYTES + 64], rnd());
  s.accounts = accounts, s.applied += n, s.batches += 1;
}
static void rollback(State &s, LedgerJournal &j, uint64_t id) {
  const long keep = j.rollback_keep(id);
  CHECK(keep >= 0);
  if (keep < 0) return;
  size_t expect_end = j.nodes();
  for (size_t c = j.calls.size(); c-- > (size_t)keep;) {
    CHECK(j.calls[c].node_begin + j.calls[c].node_count == expect_end);  // the device entries of the calls lie back to back
    expect_end = j.calls[c].node_begin;
    LedgerJournal::undo_host(j.calls[c], s.records, s.accounts, s.applied, s.batches);
  }
  j.rollback_done(id);
  CHECK(j.nodes() == expect_end);
}
static void journal() {
  for (int round = 0; round < 200; round++) {
    State s;
    LedgerJournal j;
    std::vector<std::pair<uint64_t, State>> open;  // what the journal should hold open, oldest first
    const size_t cap = 1 + rnd() % 16;
    for (int step = 0; step < 60; step++) {
      const uint64_t what = rnd() % 8;
      if (what < 4) storing_call(s, j, cap);
      else if (what == 4) {
        const uint64_t id = j.checkpoint();
        CHECK(open.empty() || id > open.back().first);
        open.push_back({id, s});
      } else if (what == 5 && !open.empty()) {  // roll back to any open checkpoint; the later ones are discarded
        const size_t at = rnd() % open.size();
        rollback(s, j, open[at].first);
        CHECK(s == open[at].second);
        for (size_t k = at + 1; k < open.size(); k++) CHECK(j.rollback_keep(open[k].first) == -1 && !j.release(open[k].first));
        open.resize(at + 1);
        if (rnd() % 2) {  // ... and again: the checkpoint stays open
          storing_call(s, j, cap);
          rollback(s, j, open[at].first);
          CHECK(s == open[at].second);
        }
      } else if (what == 6 && !open.empty()) {  // release any of them: no state moves
        const size_t at = rnd() % open.size();
        const State before = s;
        CHECK(j.release(open[at].first) && !j.release(open[at].first) && j.rollback_keep(open[at].first) == -1);
        CHECK(s == before);
        open.erase(open.begin() + at);
      } else {
        CHECK(j.rollback_keep(1000000 + rnd() % 5) == -1);  // an id never given out
      }
      CHECK(j.markers.size() == open.size() && j.open() == !open.empty());
      if (open.empty()) CHECK(j.calls.empty() && j.nodes() == 0);
    }
    while (!open.empty()) {  // what is still open can be rolled back to, the latest first
      rollback(s, j, open.back().first);
      CHECK(s == open.back().second);
      CHECK(j.release(open.back().first));
      open.pop_back();
    }
    CHECK(!j.open() && j.nodes() == 0);
  }
}

int main() {
  parser();
  journal();
  if (fails) { fprintf(stderr, "ledger_state_selfcheck: %d check(s) failed\n", fails); return 1; }
  printf("ledger_state_selfcheck: ok\n");
  return 0;
}
