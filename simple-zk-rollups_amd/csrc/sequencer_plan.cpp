// sequencer_plan.cpp -- the host passes of the transaction sequencer and of a replay (sequencer_plan.hpp) and their test hooks
// zkr_sequence_plan_host and zkr_replay_plan_host.  Reference: /root/reference/operator/src/routes/send.ts:72-135 (the operator's checks),
// prover/circuits/processtx.circom:70-193 (what the circuit then enforces; rule 6 follows the circuit).
#include "sequencer_plan.hpp"

#include <unordered_map>

#include "../../include/zkr.h"
#include "field.hpp"

namespace zkr {
void set_error(const char *fmt, ...);

bool int256_below_r(const Int256 &a) {
  for (int i = 3; i >= 0; i--) {
    const uint64_t p = (uint64_t)FrParams::P[2 * i] | ((uint64_t)FrParams::P[2 * i + 1] << 32);
    if (a.w[i] != p) return a.w[i] < p;
  }
  return false;
}

void seq_tables(unsigned depth, const std::vector<uint32_t> &idx, const uint32_t *query1, size_t n_leaves, int32_t *out) {
  const size_t U = idx.size();
  int32_t *t0 = out, *t1 = out + (size_t)depth * U, *t2 = out + 2 * (size_t)depth * U;
  std::vector<int32_t> last;
  for (unsigned l = 0; l < depth; l++) {
    // nodes of level l that an update can touch: below ((n_leaves - 1) >> l) + 1; a sibling past them was never touched
    const size_t width = n_leaves ? ((n_leaves - 1) >> l) + 1 : 0;
    last.assign(width, -1);
    auto seen = [&](size_t node) { return node < width ? last[node] : -1; };
    for (size_t u = 0; u < U; u++) {
      const size_t node = (size_t)idx[u] >> l;
      t0[l * U + u] = seen(node ^ 1);
      t1[l * U + u] = (query1 && !(u & 1)) ? seen(((size_t)query1[u / 2] >> l) ^ 1) : -1;
      last[node] = (int32_t)u;
    }
    for (size_t u = 0; u < U; u++) t2[l * U + u] = last[(size_t)idx[u] >> l] == (int32_t)u ? 1 : 0;
  }
}

int seq_plan(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *txs, size_t n_txs, const uint8_t *sig_verdicts,
             uint32_t batch, SeqPlan &out, const char **why) {
  static const char *dummy;
  if (!why) why = &dummy;
  if (depth < 1 || depth > 24) { *why = "depth out of range (1..24)"; return -1; }
  if (batch < 1) { *why = "batch must be at least 1"; return -1; }
  if (n_accounts > ((size_t)1 << depth)) { *why = "more accounts than the tree has leaves"; return -1; }
  if (n_txs > ((size_t)1 << 22)) { *why = "more than 2^22 transactions in one queue"; return -1; }
  if ((n_accounts && !records) || (n_txs && (!txs || !sig_verdicts))) { *why = "null argument"; return -1; }
  out = SeqPlan();
  out.status.assign(n_txs, SEQ_NOT_REACHED);
  std::unordered_map<uint32_t, SeqRecord> touched;  // the records the queue has changed so far
  auto record = [&](uint32_t i) {
    auto it = touched.find(i);
    if (it != touched.end()) return it->second;
    SeqRecord r;
    for (int j = 0; j < 4; j++) r.f[j] = int256_load(records + (size_t)i * 128 + 32 * j);
    return r;
  };
  auto account_of = [&](const Int256 &v, uint32_t &i) {
    if (v.w[1] | v.w[2] | v.w[3] || v.w[0] >= n_accounts) return false;
    i = (uint32_t)v.w[0];
    return true;
  };
  std::vector<uint8_t> status(n_txs);
  for (size_t t = 0; t < n_txs; t++) {
    Int256 e[8];
    for (int j = 0; j < 8; j++) e[j] = int256_load(txs + t * 256 + 32 * j);
    const Int256 &amount = e[2], &fee = e[3], &nonce = e[4];
    uint32_t from = 0, to = 0;
    uint8_t st = 0;
    if (!account_of(e[0], from)) st = 1;
    else if (!account_of(e[1], to)) st = 2;
    else {
      bool canon = int256_below_2_250(amount) && int256_below_2_250(fee) && int256_below_2_250(nonce);
      for (int j = 0; j < 8; j++) canon = canon && int256_below_r(e[j]);
      if (!canon) st = 3;
    }
    SeqRecord s{}, r{};
    if (!st) {
      s = record(from), r = record(to);
      for (int j = 0; j < 4 && !st; j++)
        if (!int256_below_r(s.f[j]) || !int256_below_r(r.f[j]) || (j >= 2 && (!int256_below_2_250(s.f[j]) || !int256_below_2_250(r.f[j])))) {
          *why = "an account record is not a field element, or its balance or nonce does not fit 250 bits";
          return -1;
        }
      const Int256 spend = int256_add(amount, fee);  // below 2^251
      if (int256_is_zero(amount)) st = 4;
      else if (int256_is_zero(fee)) st = 5;
      else if (int256_cmp(s.f[2], spend) <= 0) st = 6;
      else if (int256_cmp(fee, int256_mul_small(int256_div_small(amount, 1000), 3)) < 0) st = 7;
      else if (int256_cmp(nonce, int256_add(s.f[3], int256_small(1))) != 0) st = 8;
      else {
        SeqRecord ns = s;
        ns.f[2] = int256_sub(s.f[2], spend);
        ns.f[3] = nonce;
        SeqRecord nr = from == to ? ns : r;  // the same record when from == to (processtx.circom:141-159)
        nr.f[2] = int256_add(nr.f[2], amount);
        if (!int256_below_2_250(nr.f[2])) st = 9;
        else if (!sig_verdicts[t]) st = 10;
        else {
          out.pos.push_back((uint32_t)t);
          out.idx.push_back(from), out.idx.push_back(to);
          out.old_rec.push_back(s), out.old_rec.push_back(r);
          out.new_rec.push_back(ns), out.new_rec.push_back(nr);
          touched[from] = ns;
          touched[to] = nr;
        }
      }
    }
    status[t] = st;
  }
  // only whole batches are applied: the first A - (A mod batch) accepted transactions
  const size_t T = out.pos.size() - out.pos.size() % batch;
  out.applied = T;
  out.pos.resize(T), out.idx.resize(2 * T), out.old_rec.resize(2 * T), out.new_rec.resize(2 * T);
  out.consumed = T ? (size_t)out.pos[T - 1] + 1 : 0;
  for (size_t t = 0; t < out.consumed; t++) out.status[t] = status[t];
  out.prev.assign(3 * (size_t)depth * 2 * T, -1);
  if (T) {
    std::vector<uint32_t> to(T);
    for (size_t k = 0; k < T; k++) to[k] = out.idx[2 * k + 1];
    seq_tables(depth, out.idx, to.data(), n_accounts, out.prev.data());
  }
  return 0;
}

int replay_plan(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *publics, size_t n_batches, uint32_t batch,
                SeqPlan &out, size_t *planned, uint32_t *where, const char **why) {
  static const char *dummy;
  if (!why) why = &dummy;
  if (depth < 1 || depth > 24) { *why = "depth out of range (1..24)"; return -1; }
  if (batch < 1) { *why = "batch must be at least 1"; return -1; }
  if (n_accounts > ((size_t)1 << depth)) { *why = "more accounts than the tree has leaves"; return -1; }
  if (batch > ((size_t)1 << 22) || n_batches > ((size_t)1 << 22) / batch) { *why = "more than 2^22 transactions in one run of batches"; return -1; }
  if (!planned || !where || (n_accounts && !records) || (n_batches && !publics)) { *why = "null argument"; return -1; }
  out = SeqPlan();
  *planned = n_batches, *where = 0;
  const size_t n_public = 1 + (size_t)batch * (18 + 3 * (size_t)depth);
  std::unordered_map<uint32_t, SeqRecord> touched;  // the records the batches have changed so far
  auto record = [&](uint32_t i) {
    auto it = touched.find(i);
    if (it != touched.end()) return it->second;
    SeqRecord r;
    for (int j = 0; j < 4; j++) r.f[j] = int256_load(records + (size_t)i * 128 + 32 * j);
    return r;
  };
  auto account_of = [&](const Int256 &v, uint32_t &i) {
    if (v.w[1] | v.w[2] | v.w[3] || v.w[0] >= n_accounts) return false;
    i = (uint32_t)v.w[0];
    return true;
  };
  for (size_t b = 0; b < n_batches && *planned == n_batches; b++) {
    const uint8_t *row = publics + b * n_public * 32;
    auto refuse = [&](size_t signal) { *planned = b, *where = (uint32_t)signal; };
    for (size_t i = 0; i < n_public && *planned == n_batches; i++)
      if (!int256_below_r(int256_load(row + 32 * i))) refuse(i);
    for (uint32_t k = 0; k < batch && *planned == n_batches; k++) {
      const size_t base = 1 + (size_t)batch + 8 * (size_t)k;  // this transaction's txData row
      Int256 e[5];
      for (int j = 0; j < 5; j++) e[j] = int256_load(row + 32 * (base + j));
      const Int256 &amount = e[2], &fee = e[3], &nonce = e[4];
      uint32_t from = 0, to = 0;
      if (!account_of(e[0], from)) { refuse(base); break; }
      if (!account_of(e[1], to)) { refuse(base + 1); break; }
      if (!int256_below_2_250(amount)) { refuse(base + 2); break; }
      if (!int256_below_2_250(fee)) { refuse(base + 3); break; }
      if (!int256_below_2_250(nonce)) { refuse(base + 4); break; }
      const SeqRecord s = record(from), r = record(to);
      for (int j = 0; j < 4; j++)
        if (!int256_below_r(s.f[j]) || !int256_below_r(r.f[j]) || (j >= 2 && (!int256_below_2_250(s.f[j]) || !int256_below_2_250(r.f[j])))) {
          *why = "an account record is not a field element, or its balance or nonce does not fit 250 bits";
          return -1;
        }
      const Int256 spend = int256_add(amount, fee);  // below 2^251
      if (int256_cmp(s.f[2], spend) < 0) { refuse(base + 2); break; }
      SeqRecord ns = s;
      ns.f[2] = int256_sub(s.f[2], spend);
      ns.f[3] = nonce;
      SeqRecord nr = from == to ? ns : r;  // the same record when from == to (processtx.circom:141-159)
      nr.f[2] = int256_add(nr.f[2], amount);
      if (!int256_below_2_250(nr.f[2])) { refuse(base + 2); break; }
      out.pos.push_back((uint32_t)(b * batch + k));
      out.idx.push_back(from), out.idx.push_back(to);
      out.old_rec.push_back(s), out.old_rec.push_back(r);
      out.new_rec.push_back(ns), out.new_rec.push_back(nr);
      touched[from] = ns;
      touched[to] = nr;
    }
  }
  // a refused batch takes its first transactions with it: nothing reads `touched` after it
  const size_t T = *planned * batch;
  out.applied = out.consumed = T;
  out.pos.resize(T), out.idx.resize(2 * T), out.old_rec.resize(2 * T), out.new_rec.resize(2 * T);
  out.prev.assign(3 * (size_t)depth * 2 * T, -1);
  if (T) {
    std::vector<uint32_t> to(T);
    for (size_t k = 0; k < T; k++) to[k] = out.idx[2 * k + 1];
    seq_tables(depth, out.idx, to.data(), n_accounts, out.prev.data());
  }
  return 0;
}
}  // namespace zkr

using namespace zkr;

extern "C" int zkr_sequence_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *txs, size_t n_txs,
                                      const uint8_t *sig_verdicts, uint32_t batch, uint8_t *status, size_t *consumed, int32_t *prev) {
  if ((n_txs && !status) || !consumed) { set_error("null argument"); return ZKR_ERR_ARG; }
  SeqPlan plan;
  const char *why = "";
  if (seq_plan(depth, records, n_accounts, txs, n_txs, sig_verdicts, batch, plan, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  if (n_txs) memcpy(status, plan.status.data(), n_txs);
  *consumed = plan.consumed;
  if (prev && !plan.prev.empty()) memcpy(prev, plan.prev.data(), plan.prev.size() * sizeof(int32_t));
  return ZKR_OK;
}

extern "C" int zkr_replay_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const void *publics_std, size_t n_batches,
                                    uint32_t batch, uint8_t *verdicts, uint32_t *where, size_t *planned, uint32_t *idx, uint8_t *old_rec,
                                    uint8_t *new_rec, int32_t *prev) {
  if ((n_batches && (!verdicts || !where)) || !planned) { set_error("null argument"); return ZKR_ERR_ARG; }
  SeqPlan plan;
  const char *why = "";
  uint32_t at = 0;
  if (replay_plan(depth, records, n_accounts, (const uint8_t *)publics_std, n_batches, batch, plan, planned, &at, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  for (size_t b = 0; b < n_batches; b++) {
    verdicts[b] = b < *planned ? 0 : b == *planned ? 1 : SEQ_NOT_REACHED;
    where[b] = b == *planned ? at : 0;
  }
  const size_t U = plan.idx.size();
  if (idx && U) memcpy(idx, plan.idx.data(), U * sizeof(uint32_t));
  for (size_t u = 0; u < U; u++)
    for (int j = 0; j < 4; j++) {
      if (old_rec) int256_store(old_rec + u * 128 + 32 * j, plan.old_rec[u].f[j]);
      if (new_rec) int256_store(new_rec + u * 128 + 32 * j, plan.new_rec[u].f[j]);
    }
  if (prev && !plan.prev.empty()) memcpy(prev, plan.prev.data(), plan.prev.size() * sizeof(int32_t));
  return ZKR_OK;
}
