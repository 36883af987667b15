// sequencer_selfcheck.cpp -- a stand-alone program over zkr_sequence_plan_host and zkr_replay_plan_host (sequencer_plan.cpp: the
// host passes of the sequencer and of a replay), meant for a sanitizer build (`make sequencer-asan`: AddressSanitizer + UBSan on this file and sequencer_plan.cpp, no Python and
// no HIP in the process).  It drives the pass with generated queues over every depth and checks what must hold for ANY queue:
// statuses are rule codes, what is past `consumed` is "not reached", whole batches only, and every table entry points at an
// earlier update or at the stored tree -- the bounds the device kernels rely on.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

extern "C" int zkr_sequence_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *txs, size_t n_txs,
                                      const uint8_t *sig_verdicts, uint32_t batch, uint8_t *status, size_t *consumed, int32_t *prev);
extern "C" int zkr_replay_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const void *publics_std, size_t n_batches,
                                    uint32_t batch, uint8_t *verdicts, uint32_t *where, size_t *planned, uint32_t *idx, uint8_t *old_rec,
                                    uint8_t *new_rec, int32_t *prev);
namespace zkr {
void set_error(const char *fmt, ...) {  // the library's lives beside its HIP code
  va_list ap;
  va_start(ap, fmt);
  va_end(ap);
}
}  // namespace zkr

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fails++; fprintf(stderr, "line %d: %s\n", __LINE__, #x); } } while (0)

static uint64_t rng_state = 0x5A4B0001;
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

static void run(unsigned depth, size_t n_accounts, size_t n_txs, uint32_t batch, int wild) {
  std::vector<uint8_t> rec(n_accounts * 128 + 1), txs(n_txs * 256 + 1), verdicts(n_txs + 1, 1), status(n_txs + 1, 77);
  std::vector<uint64_t> nonce(n_accounts, 0);
  for (size_t i = 0; i < n_accounts; i++) {
    put(&rec[i * 128], 1 + i), put(&rec[i * 128 + 32], 2 + i), put(&rec[i * 128 + 64], 1000000), put(&rec[i * 128 + 96], 0);
  }
  for (size_t t = 0; t < n_txs; t++) {
    const uint64_t from = n_accounts ? rnd() % n_accounts : 0, to = n_accounts ? rnd() % n_accounts : 0;
    uint8_t *x = &txs[t * 256];
    put(x, from), put(x + 32, to), put(x + 64, 1 + rnd() % 50), put(x + 96, 1 + rnd() % 5), put(x + 128, n_accounts ? nonce[from] + 1 : 1);
    put(x + 160, rnd()), put(x + 192, rnd()), put(x + 224, rnd());
    const uint64_t kind = wild ? rnd() % 12 : 99;
    if (kind == 0) put(x, n_accounts + rnd() % 3);            // rule 1
    else if (kind == 1) put(x + 32, ~0ull);                   // rule 2
    else if (kind == 2) memset(x + 64, 0xFF, 32);             // rule 3
    else if (kind == 3) put(x + 64, 0);                       // rule 4
    else if (kind == 4) put(x + 96, 0);                       // rule 5
    else if (kind == 5) put(x + 64, 2000000);                 // rule 6
    else if (kind == 6) put(x + 128, 7 + rnd() % 3);          // rule 8 (mostly)
    else if (kind == 7) verdicts[t] = 0;                      // rule 10
    else if (n_accounts && verdicts[t]) nonce[from]++;        // what the pass will accept, unless the balance ran out
  }
  std::vector<int32_t> prev(3 * (size_t)depth * 2 * n_txs + 1, 12345);
  size_t consumed = 999999;
  const int rc = zkr_sequence_plan_host(depth, rec.data(), n_accounts, txs.data(), n_txs, verdicts.data(), batch, status.data(), &consumed, prev.data());
  CHECK(rc == 0);
  if (rc) return;
  CHECK(consumed <= n_txs && status[n_txs] == 77 && prev.back() == 12345);
  size_t T = 0;
  for (size_t t = 0; t < n_txs; t++) {
    CHECK(t < consumed ? status[t] <= 10 : status[t] == 255);
    T += status[t] == 0;
  }
  CHECK(T % batch == 0 && (T == 0) == (consumed == 0) && (consumed == 0 || status[consumed - 1] == 0));
  const size_t U = 2 * T;
  for (unsigned tb = 0; tb < 3; tb++)
    for (unsigned l = 0; l < depth; l++)
      for (size_t u = 0; u < U; u++) {
        const int32_t p = prev[((size_t)tb * depth + l) * U + u];
        if (tb == 2) CHECK(p == 0 || p == 1);
        else CHECK(p >= -1 && p < (int32_t)u);
      }
  if (U) CHECK(prev[((size_t)2 * depth) * U + U - 1] == 1);  // the last update holds the last version of its leaf
}

// The replay pass (zkr_replay_plan_host) over generated batches: `spoil` picks what is wrong with batch `bad` (0 nothing, 1 an
// index past the accounts, 2 a balance underflow, 3 a signal that is no field element).  Only txData is filled in: the pass reads
// nothing else but for the "< r" check.  Whatever the batches say, every table entry points at an earlier update or at the
// stored tree and every leaf index is an account.
static void run_replay(unsigned depth, size_t n_accounts, size_t n_batches, uint32_t batch, size_t bad, int spoil) {
  const size_t n_public = 1 + (size_t)batch * (18 + 3 * depth), room = 2 * batch * n_batches;
  std::vector<uint8_t> rec(n_accounts * 128 + 1), pub(n_batches * n_public * 32 + 1, 0), verdicts(n_batches + 1, 77);
  std::vector<uint32_t> where(n_batches + 1, 4242), idx(room + 1, 4242);
  std::vector<uint8_t> old_rec(room * 128 + 1, 0x5A), new_rec(room * 128 + 1, 0x5A);
  std::vector<int32_t> prev(3 * (size_t)depth * room + 1, 12345);
  for (size_t i = 0; i < n_accounts; i++) put(&rec[i * 128], 1 + i), put(&rec[i * 128 + 32], 2 + i), put(&rec[i * 128 + 64], 1000), put(&rec[i * 128 + 96], 0);
  size_t bad_signal = 0;
  for (size_t b = 0; b < n_batches; b++)
    for (uint32_t k = 0; k < batch; k++) {
      const size_t base = 1 + batch + 8 * (size_t)k;
      uint8_t *x = &pub[(b * n_public + base) * 32];
      const uint64_t from = rnd() % n_accounts, to = rnd() % 4 ? rnd() % n_accounts : from;  // from == to a quarter of the time
      put(x, from), put(x + 32, to), put(x + 64, rnd() % 3), put(x + 96, rnd() % 2), put(x + 128, rnd() % 5);
      put(x + 160, rnd()), put(x + 192, rnd()), put(x + 224, rnd());
      if (b != bad || k != batch - 1) continue;  // the LAST transaction of the bad batch: the ones before it must not stay applied
      if (spoil == 1) put(x + 32, n_accounts), bad_signal = base + 1;
      else if (spoil == 2) put(x + 64, 1000000), bad_signal = base + 2;
      else if (spoil == 3) memset(x + 7 * 32, 0xFF, 32), bad_signal = base + 7;
    }
  size_t planned = 999999;
  const int rc = zkr_replay_plan_host(depth, rec.data(), n_accounts, pub.data(), n_batches, batch, verdicts.data(), where.data(), &planned, idx.data(),
                                      old_rec.data(), new_rec.data(), prev.data());
  CHECK(rc == 0);
  if (rc) return;
  const size_t want = spoil && bad < n_batches ? bad : n_batches, U = 2 * batch * want;
  CHECK(planned == want && verdicts[n_batches] == 77 && where[n_batches] == 4242);
  for (size_t b = 0; b < n_batches; b++) {
    CHECK(verdicts[b] == (b < want ? 0 : b == want ? 1 : 255));
    CHECK(where[b] == (b == want ? bad_signal : 0));
  }
  CHECK(idx[U] == 4242 && old_rec[U * 128] == 0x5A && new_rec[U * 128] == 0x5A && prev[3 * (size_t)depth * U] == 12345);
  for (size_t u = 0; u < U; u++) CHECK(idx[u] < n_accounts && new_rec[u * 128 + 95] == 0);  // an account; a balance far below 2^250
  for (unsigned tb = 0; tb < 3; tb++)
    for (unsigned l = 0; l < depth; l++)
      for (size_t u = 0; u < U; u++) {
        const int32_t p = prev[((size_t)tb * depth + l) * U + u];
        if (tb == 2) CHECK(p == 0 || p == 1);
        else CHECK(p >= -1 && p < (int32_t)u);
      }
  if (U) CHECK(prev[((size_t)2 * depth) * U + U - 1] == 1);
}

int main() {
  for (unsigned depth = 1; depth <= 24; depth++) {
    const size_t accounts = (size_t)1 << (depth > 6 ? 6 : depth);
    for (uint32_t batch = 1; batch <= 3; batch++) {
      run_replay(depth, accounts, 9, batch, 99, 0);                   // every batch applies
      for (int spoil = 1; spoil <= 3; spoil++) run_replay(depth, accounts, 9, batch, 4, spoil);  // refused in the middle
      run_replay(depth, accounts, 3, batch, 0, 2);                    // the first batch: nothing planned
      run_replay(depth, accounts - 1 ? accounts - 1 : 1, 5, batch, 4, 1);  // the last batch; an account count that is no power of two
    }
    run_replay(depth, 1, 0, 1, 0, 0);                                 // no batch at all
  }
  {  // refused arguments of the replay pass
    uint8_t rec[256], pub[19 * 32 + 3 * 2 * 32] = {0}, v[1];
    uint32_t w[1];
    size_t planned;
    memset(rec, 0xFF, sizeof rec);
    put(pub + 3 * 32, 1);  // depth 2, batch 1: to = 1
    CHECK(zkr_replay_plan_host(2, rec, 2, pub, 1, 1, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);  // a record that is no field element
    CHECK(zkr_replay_plan_host(1, rec, 3, pub, 1, 1, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(0, rec, 1, pub, 1, 1, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(25, rec, 1, pub, 1, 1, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(2, rec, 2, pub, 1, 0, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(2, rec, 2, pub, ((size_t)1 << 22) + 1, 1, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(2, nullptr, 2, pub, 1, 1, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(2, rec, 2, nullptr, 1, 1, v, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(2, rec, 2, pub, 1, 1, nullptr, w, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(2, rec, 2, pub, 1, 1, v, nullptr, &planned, nullptr, nullptr, nullptr, nullptr) == -5);
    CHECK(zkr_replay_plan_host(2, rec, 2, pub, 1, 1, v, w, nullptr, nullptr, nullptr, nullptr, nullptr) == -5);
  }
  for (unsigned depth = 1; depth <= 24; depth++) {
    const size_t cap = (size_t)1 << (depth > 10 ? 10 : depth);
    for (uint32_t batch = 1; batch <= 4; batch++) {
      run(depth, cap, 200, batch, 1);
      run(depth, cap > 3 ? cap - 3 : 1, 64, batch, 0);
    }
    run(depth, 1, 5, 1, 1);
    run(depth, 0, 5, 1, 1);   // no account: every transaction breaks rule 1
    run(depth, 2, 0, 1, 1);   // an empty queue
    run(depth, 2, 3, 4096, 0);  // fewer accepted than one batch
  }
  {  // refused arguments: a record that is no field element, too many accounts, null pointers, depth and batch out of range
    uint8_t rec[256], tx[256], st[1], v[1] = {1};
    size_t consumed;
    memset(rec, 0xFF, sizeof rec);
    put(tx, 0), put(tx + 32, 1), put(tx + 64, 1), put(tx + 96, 1), put(tx + 128, 1), put(tx + 160, 1), put(tx + 192, 1), put(tx + 224, 1);
    CHECK(zkr_sequence_plan_host(2, rec, 2, tx, 1, v, 1, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(1, rec, 3, tx, 1, v, 1, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(0, rec, 1, tx, 1, v, 1, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(25, rec, 1, tx, 1, v, 1, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(2, rec, 2, tx, 1, v, 0, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(2, nullptr, 2, tx, 1, v, 1, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(2, rec, 2, nullptr, 1, v, 1, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(2, rec, 2, tx, 1, nullptr, 1, st, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(2, rec, 2, tx, 1, v, 1, nullptr, &consumed, nullptr) == -5);
    CHECK(zkr_sequence_plan_host(2, rec, 2, tx, 1, v, 1, st, nullptr, nullptr) == -5);
  }
  if (fails) { fprintf(stderr, "sequencer_selfcheck: %d check(s) failed\n", fails); return 1; }
  printf("sequencer_selfcheck: ok\n");
  return 0;
}
