// book_selfcheck.cpp -- a stand-alone program over the host side of the ledger's book (book_plan.cpp: the deposit and withdraw
// passes and the ZKRBOOK1 parser), meant for a sanitizer build (`make book-asan`: AddressSanitizer + UBSan on this file,
// book_plan.cpp, sequencer_plan.cpp and rollup.cpp, which has the tag's hash; no Python and no HIP in the process).  It plays the
// cases of tests/test_book_cpu.py -- every status and verdict, the duplicates of one list, resolve results that cannot be true --
// and generated lists, each buffer in an allocation of exactly its length, and feeds the parser good blobs and blobs damaged one
// field at a time.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "../../include/zkr.h"
#include "book_plan.hpp"

extern "C" int zkr_book_deposit_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *pubs, const uint8_t *values, size_t n,
                                          const uint32_t *resolved, uint8_t *status, uint32_t *indices, uint8_t *events);
extern "C" int zkr_book_withdraw_plan_host(const uint8_t *records, size_t n_accounts, const uint8_t *publics, const uint8_t *amounts, const uint8_t *proof_verdicts,
                                           size_t n, const uint32_t *resolved, uint8_t *verdicts, uint32_t *indices, uint8_t *events);
extern "C" int zkr_book_blob_check(const void *blob, size_t len, uint64_t info[2], int *valid);
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

static uint64_t rng_state = 0x5A4B000B;
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
static uint64_t low(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
static const uint8_t R_LE[32] = {0x01, 0x00, 0x00, 0xf0, 0x93, 0xf5, 0xe1, 0x43, 0x91, 0x70, 0xb9, 0x79, 0x48, 0xe8, 0x33, 0x28,
                                 0x5d, 0x58, 0x81, 0x81, 0xb6, 0x45, 0x50, 0xb8, 0x29, 0xa0, 0x31, 0xe1, 0x72, 0x4e, 0x64, 0x30};  // r
static const uint32_t ALL = BOOK_X_BELOW_R | BOOK_Y_BELOW_R | BOOK_NULL_BELOW_R;

struct Accounts {  // account i holds key (100 + i, 200 + i)
  std::vector<uint8_t> rec;
  explicit Accounts(size_t n, uint64_t balance) : rec(n * 128) {
    for (size_t i = 0; i < n; i++) put(&rec[i * 128], 100 + i), put(&rec[i * 128 + 32], 200 + i), put(&rec[i * 128 + 64], balance), put(&rec[i * 128 + 96], 3);
  }
  size_t n() const { return rec.size() / 128; }
};

static void deposits() {
  Accounts a(3, 50);  // depth 2: one leaf left
  // 0: existing key; 1: new key; 2: the same new key again; 3: another new key, tree full; 4: key not below r; 5: value 2^250;
  // 6: balance would reach 2^250
  const size_t n = 7;
  std::vector<uint8_t> pubs(n * 64), values(n * 32), status(n, 77), events(n * 128, 0xEE);
  std::vector<uint32_t> res(3 * n), idx(n, 5);
  const uint64_t kx[n] = {101, 900, 900, 901, 0, 100, 102};
  for (size_t i = 0; i < n; i++) put(&pubs[i * 64], kx[i]), put(&pubs[i * 64 + 32], kx[i] + 100), put(&values[i * 32], 10 + i);
  memcpy(&pubs[4 * 64], R_LE, 32);
  memset(&values[5 * 32], 0, 32), values[5 * 32 + 31] = 0x04;
  memset(&values[6 * 32], 0xFF, 31), values[6 * 32 + 31] = 0x03;  // 2^250 - 1
  const uint32_t acct[n] = {1, BOOK_NONE, BOOK_NONE, BOOK_NONE, BOOK_NONE, 0, 2}, lead[n] = {0, 1, 1, 3, 4, 5, 6};
  for (size_t i = 0; i < n; i++) res[3 * i] = i == 4 ? BOOK_Y_BELOW_R : ALL, res[3 * i + 1] = acct[i], res[3 * i + 2] = lead[i];
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), pubs.data(), values.data(), n, res.data(), status.data(), idx.data(), events.data()) == 0);
  const uint8_t want[n] = {0, 0, 0, 2, 1, 1, 3};
  for (size_t i = 0; i < n; i++) CHECK(status[i] == want[i]);
  CHECK(idx[0] == 1 && idx[1] == 3 && idx[2] == 3 && idx[3] == BOOK_NONE && idx[6] == BOOK_NONE);
  CHECK(low(&events[0 * 128 + 64]) == 60 && low(&events[0 * 128 + 96]) == 3);
  CHECK(low(&events[1 * 128 + 64]) == 11 && low(&events[2 * 128 + 64]) == 23 && low(&events[2 * 128 + 96]) == 0 && low(&events[2 * 128]) == 900);
  for (size_t j = 0; j < 128; j++) CHECK(events[3 * 128 + j] == 0);
  // a leader that was refused: the later copy is the one that creates the account
  put(&values[1 * 32], 0), values[1 * 32 + 31] = 0x04;
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), pubs.data(), values.data(), n, res.data(), status.data(), idx.data(), nullptr) == 0);
  CHECK(status[1] == 1 && status[2] == 0 && idx[2] == 3 && status[3] == 2);
  // resolve results that cannot be true are refused, not followed
  std::vector<uint32_t> bad(res);
  bad[1] = 7;  // no such account
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), pubs.data(), values.data(), n, bad.data(), status.data(), idx.data(), nullptr) == ZKR_ERR_ARG);
  bad = res, bad[1] = 2;  // an account under another key
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), pubs.data(), values.data(), n, bad.data(), status.data(), idx.data(), nullptr) == ZKR_ERR_ARG);
  bad = res, bad[3 * 2 + 2] = 5;  // a leader behind its entry
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), pubs.data(), values.data(), n, bad.data(), status.data(), idx.data(), nullptr) == ZKR_ERR_ARG);
  bad = res, bad[3 * 2 + 2] = 0;  // a leader with another key
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), pubs.data(), values.data(), n, bad.data(), status.data(), idx.data(), nullptr) == ZKR_ERR_ARG);
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0);
  CHECK(zkr_book_deposit_plan_host(2, a.rec.data(), a.n(), nullptr, values.data(), n, res.data(), status.data(), nullptr, nullptr) == ZKR_ERR_ARG);
}

static void withdrawals() {
  Accounts a(4, 50);
  // 0: not below r; 1: in the set; 2: proof refused; 3: unknown key; 4: amount above the balance; 5: applied (40 of 50);
  // 6: the same nullifier as 4 -- 4 was refused, so this one is applied; 7: the same again: used; 8: 11 of the 10 left
  const size_t n = 9;
  std::vector<uint8_t> pub(n * 96), amounts(n * 32), proofs(n, 0), verdicts(n, 77), events(n * 128, 0xEE);
  std::vector<uint32_t> res(3 * n), idx(n, 5);
  const uint64_t who[n] = {0, 0, 0, 9, 1, 2, 1, 1, 2}, nul[n] = {1000, 1001, 1002, 1003, 1004, 1005, 1004, 1004, 1008}, amt[n] = {1, 1, 1, 1, 51, 40, 50, 0, 11};
  const uint32_t lead[n] = {0, 1, 2, 3, 4, 5, 4, 4, 8};
  for (size_t i = 0; i < n; i++) {
    put(&pub[i * 96], 100 + who[i]), put(&pub[i * 96 + 32], 200 + who[i]), put(&pub[i * 96 + 64], nul[i]), put(&amounts[i * 32], amt[i]);
    res[3 * i] = ALL, res[3 * i + 1] = who[i] < 4 ? (uint32_t)who[i] : BOOK_NONE, res[3 * i + 2] = lead[i];
  }
  memcpy(&pub[0 * 96 + 64], R_LE, 32), res[0] = BOOK_X_BELOW_R | BOOK_Y_BELOW_R;
  res[3 * 1] |= BOOK_NULL_USED;
  proofs[2] = 1;
  CHECK(zkr_book_withdraw_plan_host(a.rec.data(), a.n(), pub.data(), amounts.data(), proofs.data(), n, res.data(), verdicts.data(), idx.data(), events.data()) == 0);
  const uint8_t want[n] = {1, 2, 3, 4, 5, 0, 0, 2, 5};
  for (size_t i = 0; i < n; i++) CHECK(verdicts[i] == want[i]);
  CHECK(idx[5] == 2 && low(&events[5 * 128 + 64]) == 10 && idx[6] == 1 && low(&events[6 * 128 + 64]) == 0 && low(&events[6 * 128 + 96]) == 3 && idx[7] == BOOK_NONE);
  // withdrawAll: everything, then nothing is left
  std::vector<uint32_t> r2 = {ALL, 3, 0, ALL, 3, 1};
  std::vector<uint8_t> p2(2 * 96);
  for (size_t i = 0; i < 2; i++) put(&p2[i * 96], 103), put(&p2[i * 96 + 32], 203), put(&p2[i * 96 + 64], 7 + i);
  CHECK(zkr_book_withdraw_plan_host(a.rec.data(), a.n(), p2.data(), nullptr, nullptr, 2, r2.data(), verdicts.data(), idx.data(), events.data()) == 0);
  CHECK(verdicts[0] == 0 && verdicts[1] == 6 && low(&events[64]) == 0);
  std::vector<uint32_t> bad(res);
  bad[3 * 6 + 2] = 5;  // a leader with another nullifier
  CHECK(zkr_book_withdraw_plan_host(a.rec.data(), a.n(), pub.data(), amounts.data(), nullptr, n, bad.data(), verdicts.data(), idx.data(), nullptr) == ZKR_ERR_ARG);
  bad = res, bad[3 * 5 + 1] = 3;  // an account under another key
  CHECK(zkr_book_withdraw_plan_host(a.rec.data(), a.n(), pub.data(), amounts.data(), nullptr, n, bad.data(), verdicts.data(), idx.data(), nullptr) == ZKR_ERR_ARG);
  bad = res, bad[3 * 5 + 1] = 4;  // no such account
  CHECK(zkr_book_withdraw_plan_host(a.rec.data(), a.n(), pub.data(), amounts.data(), nullptr, n, bad.data(), verdicts.data(), idx.data(), nullptr) == ZKR_ERR_ARG);
}

// Generated lists over a true resolve result: what must hold for ANY list.
static void generated(size_t n_accounts, size_t n) {
  Accounts a(n_accounts, 100);
  std::vector<uint8_t> pub(n * 96 + 1), amounts(n * 32 + 1), verdicts(n + 1, 77), events(n * 128 + 1);
  std::vector<uint32_t> res(3 * n + 1), idx(n + 1), first_of(64, BOOK_NONE);
  for (size_t i = 0; i < n; i++) {
    const uint64_t who = rnd() % (n_accounts + 2), nul = rnd() % 64;
    put(&pub[i * 96], 100 + who), put(&pub[i * 96 + 32], 200 + who), put(&pub[i * 96 + 64], nul), put(&amounts[i * 32], rnd() % 60);
    if (first_of[nul] == BOOK_NONE) first_of[nul] = (uint32_t)i;
    res[3 * i] = ALL | (nul < 4 ? BOOK_NULL_USED : 0), res[3 * i + 1] = who < n_accounts ? (uint32_t)who : BOOK_NONE, res[3 * i + 2] = first_of[nul];
  }
  CHECK(zkr_book_withdraw_plan_host(a.rec.data(), n_accounts, pub.data(), amounts.data(), nullptr, n, res.data(), verdicts.data(), idx.data(), events.data()) == 0);
  std::vector<uint64_t> balance(n_accounts, 100);
  std::vector<uint8_t> spent(64, 0);
  for (size_t i = 0; i < n; i++) {
    const uint64_t nul = low(&pub[i * 96 + 64]);
    CHECK(verdicts[i] <= 6 && verdicts[i] != 1 && verdicts[i] != 3 && verdicts[i] != 6);
    CHECK((verdicts[i] == 0) == (idx[i] != BOOK_NONE));
    if (verdicts[i] == 2) CHECK(nul < 4 || spent[nul]);
    if (verdicts[i]) continue;
    CHECK(!spent[nul] && nul >= 4 && idx[i] < n_accounts);
    spent[nul] = 1;
    balance[idx[i]] -= low(&amounts[i * 32]);
    CHECK(low(&events[i * 128 + 64]) == balance[idx[i]] && balance[idx[i]] <= 100);
  }
  // the same keys as deposits: every new key gets one account, in order of first appearance
  std::vector<uint8_t> pubs(n * 64 + 1), status(n + 1);
  std::vector<uint32_t> first_key(n_accounts + 2, BOOK_NONE);
  for (size_t i = 0; i < n; i++) {
    memcpy(&pubs[i * 64], &pub[i * 96], 64);
    const uint64_t who = low(&pub[i * 96]) - 100;
    if (first_key[who] == BOOK_NONE) first_key[who] = (uint32_t)i;
    res[3 * i + 2] = first_key[who];
  }
  CHECK(zkr_book_deposit_plan_host(10, a.rec.data(), n_accounts, pubs.data(), amounts.data(), n, res.data(), status.data(), idx.data(), events.data()) == 0);
  for (size_t i = 0; i < n; i++) {
    const uint64_t who = low(&pub[i * 96]) - 100;
    uint64_t want = who;
    if (who >= n_accounts) want = n_accounts + (first_key[who == n_accounts ? n_accounts + 1 : n_accounts] < first_key[who] ? 1 : 0);
    CHECK(status[i] == 0 && idx[i] == want);
  }
}

static std::vector<uint8_t> blob_of(uint64_t count, uint64_t fees_lo, uint64_t fees_hi) {
  std::vector<uint8_t> b(BOOK_HEADER_BYTES + 32 * count);
  BookHeader h;
  h.count = count;
  memcpy(h.fees, &fees_lo, 8), memcpy(h.fees + 24, &fees_hi, 8);
  CHECK(book_header_write(h, b.data()) == 0);
  for (uint64_t i = 0; i < count; i++) put(&b[BOOK_HEADER_BYTES + 32 * i], rnd());
  return b;
}
// the check over a copy that is exactly `len` bytes long, so that a read past the end is an error the sanitizer sees
static bool refused(const std::vector<uint8_t> &blob, const char *word) {
  std::vector<uint8_t> exact(blob);
  exact.shrink_to_fit();
  uint64_t info[2] = {7, 7};
  int valid = 7;
  last_error[0] = 0;
  const int rc = zkr_book_blob_check(exact.data(), exact.size(), info, &valid);
  return rc == 0 && valid == 0 && info[0] == 7 && strstr(last_error, word) != nullptr;
}
static void parser() {
  for (uint64_t count : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)33}) {
    std::vector<uint8_t> b = blob_of(count, 12345 + count, count ? ~0ull : 0);
    uint64_t info[2];
    int valid = 0;
    CHECK(zkr_book_blob_check(b.data(), b.size(), info, &valid) == 0 && valid == 1 && info[0] == count && info[1] == b.size());
    std::vector<uint8_t> d = b;
    d[0] ^= 1;
    CHECK(refused(d, "magic"));
    d = b, d[8] ^= 1;
    CHECK(refused(d, "length"));
    d = b, d[20] = 1;
    CHECK(refused(d, "reserved"));
    d = b, d[64] ^= 1;
    CHECK(refused(d, "tag"));
    d = b, d[95] ^= 0x80;
    CHECK(refused(d, "tag"));
    d = b, d[100] ^= 1;
    CHECK(refused(d, "tag"));
    d = b, d.push_back(0);
    CHECK(refused(d, "length"));
    d = b, d.resize(b.size() - 1);
    CHECK(refused(d, count ? "length" : "shorter"));
    d = b, d.resize(10);
    CHECK(refused(d, "shorter"));
    if (count) {
      d = b, memcpy(&d[BOOK_HEADER_BYTES + 32 * (count - 1)], R_LE, 32);
      CHECK(refused(d, "not below r"));
      d[BOOK_HEADER_BYTES + 32 * (count - 1)] = 0;  // r - 1
      CHECK(zkr_book_blob_check(d.data(), d.size(), info, &valid) == 0 && valid == 1);
    }
  }
  uint64_t info[2];
  int valid = 3;
  CHECK(zkr_book_blob_check(nullptr, 0, info, &valid) == ZKR_ERR_ARG && valid == 0);
}

int main() {
  deposits();
  withdrawals();
  for (size_t n_accounts : {(size_t)0, (size_t)1, (size_t)5})
    for (size_t n : {(size_t)1, (size_t)2, (size_t)64, (size_t)300}) generated(n_accounts, n);
  parser();
  if (fails) { fprintf(stderr, "book_selfcheck: %d failure(s)\n", fails); return 1; }
  printf("book_selfcheck: ok\n");
  return 0;
}
