// book_plan.cpp -- the host pass of the ledger's book (book_plan.hpp), the ZKRBOOK1 blob, and the host-only calls
// zkr_book_deposit_plan_host, zkr_book_withdraw_plan_host and zkr_book_blob_check.  Reference:
// contracts/contracts/RollUp.sol:193-309 of the reference.  Nothing here touches a device.
#include "book_plan.hpp"

#include <stdio.h>
#include <unordered_map>

#include "../../include/zkr.h"

namespace zkr {
void set_error(const char *fmt, ...);

namespace {
struct Touched {  // balances as the list has left them so far; an account the list has not touched stands in the records
  const uint8_t *records;
  size_t n_accounts;
  std::unordered_map<uint32_t, SeqRecord> now;
  SeqRecord get(uint32_t idx) const {
    auto it = now.find(idx);
    if (it != now.end()) return it->second;
    SeqRecord r;
    for (int j = 0; j < 4; j++) r.f[j] = int256_load(records + (size_t)idx * 128 + 32 * j);
    return r;
  }
};
void emit(BookPlan &out, size_t i, uint32_t idx, const SeqRecord &rec) {
  uint8_t raw[128];
  for (int j = 0; j < 4; j++) int256_store(raw + 32 * j, rec.f[j]);
  out.index[i] = idx;
  memcpy(&out.events[i * 128], raw, 128);
  out.upd_idx.push_back(idx);
  out.upd_rec.insert(out.upd_rec.end(), raw, raw + 128);
}
void start(BookPlan &out, size_t n, size_t n_accounts) {
  out = BookPlan();
  out.status.assign(n, 0);
  out.index.assign(n, BOOK_NONE);
  out.events.assign(n * 128, 0);
  out.accounts_after = n_accounts;
}
}  // namespace

int deposit_plan(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *pubs, const uint8_t *values, size_t n,
                 const BookResolve *res, BookPlan &out, const char **why) {
  start(out, n, n_accounts);
  if (depth < 1 || depth > 24 || n_accounts > ((size_t)1 << depth)) { *why = "deposit calls: the accounts do not fit the tree"; return -1; }
  Touched t{records, n_accounts, {}};
  std::vector<uint32_t> new_of(n, BOOK_NONE);  // by leader: the index the list gave its key, once a call under it was applied
  size_t accounts = n_accounts;
  for (size_t i = 0; i < n; i++) {
    const BookResolve &r = res[i];
    const Int256 value = int256_load(values + i * 32);
    if (!(r.flags & BOOK_X_BELOW_R) || !(r.flags & BOOK_Y_BELOW_R) || !int256_below_2_250(value)) { out.status[i] = DEP_RANGE; continue; }
    uint32_t idx = r.account;
    bool fresh = false;
    if (idx != BOOK_NONE) {
      if (idx >= n_accounts || memcmp(records + (size_t)idx * 128, pubs + i * 64, 64)) { *why = "internal: the key table names an account that does not hold the call's key"; return -1; }
    } else {
      if (r.leader > i || memcmp(pubs + (size_t)r.leader * 64, pubs + i * 64, 64)) { *why = "internal: a deposit call's leader does not hold its key"; return -1; }
      idx = new_of[r.leader];
      if (idx == BOOK_NONE) {
        if (accounts == ((size_t)1 << depth)) { out.status[i] = DEP_FULL; continue; }
        idx = (uint32_t)accounts, fresh = true;
      }
    }
    SeqRecord rec;
    if (fresh) {
      rec.f[0] = int256_load(pubs + i * 64), rec.f[1] = int256_load(pubs + i * 64 + 32);
      rec.f[2] = rec.f[3] = int256_small(0);
    } else rec = t.get(idx);
    const Int256 sum = int256_add(rec.f[2], value);  // both below 2^250
    if (!int256_below_2_250(sum)) { out.status[i] = DEP_BALANCE; continue; }
    rec.f[2] = sum;
    if (fresh) new_of[r.leader] = idx, accounts++;
    t.now[idx] = rec;
    emit(out, i, idx, rec);
  }
  out.accounts_after = accounts;
  return 0;
}

int withdraw_plan(const uint8_t *records, size_t n_accounts, const uint8_t *publics, const uint8_t *amounts, const uint8_t *proof_verdicts,
                  size_t n, const BookResolve *res, BookPlan &out, const char **why) {
  start(out, n, n_accounts);
  Touched t{records, n_accounts, {}};
  std::vector<uint8_t> spent(n, 0);  // by leader: an earlier call of this list with the same nullifier was applied
  const uint32_t in_range = BOOK_X_BELOW_R | BOOK_Y_BELOW_R | BOOK_NULL_BELOW_R;
  for (size_t i = 0; i < n; i++) {
    const BookResolve &r = res[i];
    if ((r.flags & in_range) != in_range) { out.status[i] = WD_RANGE; continue; }
    if (r.leader > i || memcmp(publics + (size_t)r.leader * 96 + 64, publics + i * 96 + 64, 32)) { *why = "internal: a withdraw call's leader does not hold its nullifier"; return -1; }
    if ((r.flags & BOOK_NULL_USED) || spent[r.leader]) { out.status[i] = WD_USED; continue; }
    if (proof_verdicts && proof_verdicts[i]) { out.status[i] = WD_PROOF; continue; }
    if (r.account == BOOK_NONE) { out.status[i] = WD_NO_KEY; continue; }
    const uint32_t idx = r.account;
    if (idx >= n_accounts || memcmp(records + (size_t)idx * 128, publics + i * 96, 64)) { *why = "internal: the key table names an account that does not hold the call's key"; return -1; }
    SeqRecord rec = t.get(idx);
    Int256 amount;
    if (amounts) {
      amount = int256_load(amounts + i * 32);
      if (int256_cmp(amount, rec.f[2]) > 0) { out.status[i] = WD_AMOUNT; continue; }
    } else {
      if (int256_is_zero(rec.f[2])) { out.status[i] = WD_ZERO; continue; }
      amount = rec.f[2];
    }
    rec.f[2] = int256_sub(rec.f[2], amount);
    t.now[idx] = rec;
    spent[r.leader] = 1;
    out.accepted.push_back((uint32_t)i);
    emit(out, i, idx, rec);
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ the ZKRBOOK1 blob
static const char BOOK_MAGIC[9] = "ZKRBOOK1";
static void put_u64(uint8_t *p, uint64_t v) { for (int i = 0; i < 8; i++) p[i] = (uint8_t)(v >> (8 * i)); }
static uint64_t get_u64(const uint8_t *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)p[i] << (8 * i); return v; }

// tag = multiHash(count, low 128 bits of the fees, high 128 bits): the counter is any 256-bit number, the hash takes field elements
static int book_tag(const BookHeader &h, uint8_t tag[32]) {
  uint8_t in[3 * 32] = {0};
  put_u64(in, h.count);
  memcpy(in + 32, h.fees, 16), memcpy(in + 64, h.fees + 16, 16);
  return zkr_mimcsponge_multihash(in, 3, tag) == ZKR_OK ? 0 : -1;
}

int book_header_write(const BookHeader &h, uint8_t out[BOOK_HEADER_BYTES]) {
  memset(out, 0, BOOK_HEADER_BYTES);
  memcpy(out, BOOK_MAGIC, 8);
  put_u64(out + 8, h.count);
  memcpy(out + 64, h.fees, 32);
  return book_tag(h, out + 96);
}

int book_blob_parse(const uint8_t *blob, size_t len, BookHeader *h, char *why, size_t why_len) {
#define refuse(...) (snprintf(why, why_len, __VA_ARGS__), -1)
  if (len < BOOK_HEADER_BYTES) return refuse("book blob: length %zu is shorter than the %zu header bytes", len, (size_t)BOOK_HEADER_BYTES);
  if (memcmp(blob, BOOK_MAGIC, 8)) return refuse("book blob: wrong magic (not ZKRBOOK1)");
  for (size_t i = 16; i < 64; i++)
    if (blob[i]) return refuse("book blob: reserved byte at offset %zu is not zero", i);
  BookHeader hd;
  hd.count = get_u64(blob + 8);
  memcpy(hd.fees, blob + 64, 32);
  if (hd.count > ((uint64_t)1 << 40) || len != BOOK_HEADER_BYTES + 32 * (size_t)hd.count)
    return refuse("book blob: length %zu, but %llu nullifiers make %llu bytes", len, (unsigned long long)hd.count, (unsigned long long)(BOOK_HEADER_BYTES + 32 * hd.count));
  uint8_t tag[32];
  if (book_tag(hd, tag)) return refuse("book blob: the tag could not be computed");
  if (memcmp(tag, blob + 96, 32)) return refuse("book blob: the tag does not match the header (the count or the fees were changed)");
  for (size_t i = 0; i < (size_t)hd.count; i++)
    if (!int256_below_r(int256_load(blob + BOOK_HEADER_BYTES + 32 * i))) return refuse("book blob: nullifier %zu is not below r", i);
#undef refuse
  *h = hd;
  return 0;
}

}  // namespace zkr

using namespace zkr;

static void plan_out(const BookPlan &plan, size_t n, uint8_t *status, uint32_t *indices, uint8_t *events) {
  if (!n) return;
  memcpy(status, plan.status.data(), n);
  if (indices) memcpy(indices, plan.index.data(), n * sizeof(uint32_t));
  if (events) memcpy(events, plan.events.data(), n * 128);
}

extern "C" int zkr_book_deposit_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *pubs, const uint8_t *values, size_t n,
                                          const uint32_t *resolved, uint8_t *status, uint32_t *indices, uint8_t *events) {
  if ((n_accounts && !records) || (n && (!pubs || !values || !resolved || !status))) { set_error("null argument"); return ZKR_ERR_ARG; }
  BookPlan plan;
  const char *why = "";
  if (deposit_plan(depth, records, n_accounts, pubs, values, n, (const BookResolve *)resolved, plan, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  plan_out(plan, n, status, indices, events);
  return ZKR_OK;
}

extern "C" int zkr_book_withdraw_plan_host(const uint8_t *records, size_t n_accounts, const uint8_t *publics, const uint8_t *amounts, const uint8_t *proof_verdicts,
                                           size_t n, const uint32_t *resolved, uint8_t *verdicts, uint32_t *indices, uint8_t *events) {
  if ((n_accounts && !records) || (n && (!publics || !resolved || !verdicts))) { set_error("null argument"); return ZKR_ERR_ARG; }
  BookPlan plan;
  const char *why = "";
  if (withdraw_plan(records, n_accounts, publics, amounts, proof_verdicts, n, (const BookResolve *)resolved, plan, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  plan_out(plan, n, verdicts, indices, events);
  return ZKR_OK;
}

extern "C" int zkr_book_blob_check(const void *blob, size_t len, uint64_t info[2], int *valid) {
  if (valid) *valid = 0;
  if (!blob || !info || !valid) { set_error("null argument"); return ZKR_ERR_ARG; }
  BookHeader h;
  char why[200];
  if (book_blob_parse((const uint8_t *)blob, len, &h, why, sizeof why)) { set_error("%s", why); return ZKR_OK; }
  info[0] = h.count, info[1] = BOOK_HEADER_BYTES + 32 * h.count;
  *valid = 1;
  return ZKR_OK;
}
