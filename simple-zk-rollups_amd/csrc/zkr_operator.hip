// zkr_operator.hip -- one operator step behind one handle (include/zkr.h zkr_operator_*): a queue of signed
// transactions in; statuses, proofs and public signals out; the ledger moves only when every proof of the step is good.
// No kernel lives here.  The step is the existing calls in the order a caller would make them -- zkr_ledger_sequence,
// zkr_rollup_witness_batch_from_device, zkr_r1cs_check_device, zkr_prove_batch_device, zkr_verify_each_device -- over device
// buffers the handle owns, inside a ledger checkpoint the handle opens and closes.  A host language without a device allocator
// (the Node binding) therefore needs host buffers only.
#include <chrono>
#include <mutex>
#include <string>
#include "ledger_internal.hpp"

using namespace zkr;

struct zkr_operator {
  zkr_ledger *ledger = nullptr;  // the four handles are borrowed: the caller keeps them alive longer than the operator
  zkr_key *key = nullptr;
  zkr_r1cs *cs = nullptr;
  zkr_vk *vk = nullptr;
  int device = 0;
  uint32_t batch = 0, depth = 0, n_vars = 0, n_public = 0, max_batches = 0;
  size_t cap = 0;                 // batches the three buffers below have room for; grows to the largest step seen
  Dev<uint8_t> d_inputs, d_wit;   // cap x (nPublic - 1) x 32 B as zkr_ledger_sequence writes them; cap x nVars x 32 B
  Pinned<const void *> ptrs;      // cap device pointers, witness b = d_wit + b x nVars x 32: what the four device calls take
  OwnStream stream;               // sequencing and witnesses run here; check, proof and verdicts start behind it
  double ms[6] = {0, 0, 0, 0, 0, 0};
  std::mutex mu;                  // one step at a time
  size_t in_bytes() const { return (size_t)(n_public - 1) * 32; }
  size_t wit_bytes() const { return (size_t)n_vars * 32; }
};

namespace {

constexpr uint32_t DEFAULT_MAX_BATCHES = 256;

int reserve(zkr_operator *op, size_t n_batches) {
  if (n_batches <= op->cap) return ZKR_OK;
  op->cap = 0;  // the old blocks go first: a step keeps nothing between calls
  int rc;
  if ((rc = op->d_inputs.alloc(n_batches * op->in_bytes())) || (rc = op->d_wit.alloc(n_batches * op->wit_bytes())) || (rc = op->ptrs.alloc(n_batches))) return rc;
  for (size_t b = 0; b < n_batches; b++) op->ptrs[b] = (uint8_t *)op->d_wit + b * op->wit_bytes();
  op->cap = n_batches;
  return ZKR_OK;
}

// The ledger back at the step's checkpoint and the checkpoint gone; `rc` and its message are what the caller sees.  Both calls
// succeed on a ledger whose checkpoint this step opened; a failure of theirs (a HIP error) replaces the message.
int undo(zkr_operator *op, uint64_t cp, int rc) {
  const std::string why = zkr_last_error();
  if (int r2 = zkr_ledger_rollback(op->ledger, cp)) return r2;
  if (int r2 = zkr_ledger_release(op->ledger, cp)) return r2;
  set_error("%s", why.c_str());
  return rc;
}

struct StepClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void mark(double &slot) {  // every stage of a step returns synchronised: wall time is the stage's time
    const auto t1 = std::chrono::steady_clock::now();
    slot = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
  }
};

}  // namespace

extern "C" {

int zkr_operator_new(zkr_ledger *l, zkr_key *key, zkr_r1cs *cs, zkr_vk *vk, const zkr_operator_opts *opts, zkr_operator **out) {
  if (!l || !key || !opts || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  *out = nullptr;
  if (opts->flags || opts->reserved) { set_error("operator options: flags and reserved must be 0"); return ZKR_ERR_ARG; }
  // every check before anything is allocated
  const int device = zkr_key_device(key);
  if (l->device != device) { set_error("the ledger is on device %d, the key on device %d", l->device, device); return ZKR_ERR_ARG; }
  uint64_t vki[2] = {0, 0};
  if (vk) {
    if (int rc = zkr_vk_info(vk, vki)) return rc;
    if ((int)vki[1] != device) { set_error("the verifying key is on device %d, the key on device %d", (int)vki[1], device); return ZKR_ERR_ARG; }
  }
  uint64_t ki[10];
  if (int rc = zkr_key_info(key, ki)) return rc;
  uint32_t n_vars = 0, n_public = 0, n_constraints = 0;
  if (int rc = zkr_rollup_info(opts->batch, l->depth, &n_vars, &n_public, &n_constraints)) return rc;
  if (n_vars != ki[0] || n_public != ki[1]) {
    set_error("BatchProcessTx(%u, %u) -- the batch asked for and the ledger's depth -- has nVars=%u nPublic=%u, the key nVars=%llu nPublic=%llu", opts->batch,
              l->depth, n_vars, n_public, (unsigned long long)ki[0], (unsigned long long)ki[1]);
    return ZKR_ERR_ARG;
  }
  if (cs) {
    int same = 0;
    if (int rc = zkr_r1cs_matches_key(cs, key, &same)) return rc;  // names the devices when they differ
    if (!same) {
      const std::string why = zkr_last_error();
      set_error("the constraint system is not the key's: %s", why.c_str());
      return ZKR_ERR_ARG;
    }
  }
  if (vk && vki[0] != n_public) {
    set_error("the verifying key has nPublic=%llu, the key nPublic=%u", (unsigned long long)vki[0], n_public);
    return ZKR_ERR_ARG;
  }
  if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed", device); return ZKR_ERR_HIP; }
  zkr_operator *op = new zkr_operator();
  op->ledger = l; op->key = key; op->cs = cs; op->vk = vk;
  op->device = device;
  op->batch = opts->batch; op->depth = l->depth; op->n_vars = n_vars; op->n_public = n_public;
  op->max_batches = opts->max_batches ? opts->max_batches : DEFAULT_MAX_BATCHES;
  int rc;
  if ((rc = op->stream.create()) || (rc = reserve(op, 1))) { delete op; return rc; }  // zkr_ledger_sequence wants a buffer for a queue without a whole batch too
  *out = op;
  return ZKR_OK;
}

void zkr_operator_free(zkr_operator *op) {
  if (!op) return;
  (void)hipSetDevice(op->device);
  delete op;
}

int zkr_operator_info(const zkr_operator *op, uint64_t out[6]) {
  if (!op || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  out[0] = op->batch; out[1] = op->depth; out[2] = op->n_vars; out[3] = op->n_public; out[4] = op->max_batches;
  out[5] = op->cap * (op->in_bytes() + op->wit_bytes());
  return ZKR_OK;
}

int zkr_operator_stage_times(const zkr_operator *op, double ms[6]) {
  if (!op || !ms) { set_error("null argument"); return ZKR_ERR_ARG; }
  for (int i = 0; i < 6; i++) ms[i] = op->ms[i];
  return ZKR_OK;
}

int zkr_operator_step(zkr_operator *op, const uint8_t *txs, size_t n_txs, const uint8_t *r32s, const uint8_t *s32s, uint8_t *status, uint8_t *proofs_out,
                      void *publics_out, size_t *n_batches, size_t *consumed) {
  if (!op || !n_batches || !consumed || (n_txs && (!txs || !status))) { set_error("null argument"); return ZKR_ERR_ARG; }
  *n_batches = 0, *consumed = 0;
  const size_t room = n_txs / op->batch;  // the most batches the queue can fill
  if (room && (!proofs_out || !publics_out)) { set_error("null argument"); return ZKR_ERR_ARG; }
  if ((r32s == nullptr) != (s32s == nullptr)) { set_error("r32s and s32s: both or neither"); return ZKR_ERR_ARG; }
  if (room > op->max_batches) {
    set_error("%zu transactions can fill %zu batches of %u, the operator takes %u in one step", n_txs, room, op->batch, op->max_batches);
    return ZKR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(op->mu);
  ZKR_HIP_CHECK(hipSetDevice(op->device));
  if (int rc = reserve(op, room)) return rc;
  for (double &m : op->ms) m = 0;
  zkr_ledger *l = op->ledger;
  const hipStream_t st = op->stream;
  uint64_t cp = 0;
  if (int rc = zkr_ledger_checkpoint(l, &cp)) return rc;
  StepClock clk;

  size_t nb = 0;
  if (int rc = zkr_ledger_sequence(l, txs, n_txs, op->batch, status, op->d_inputs, &nb, consumed, st)) {
    const std::string why = zkr_last_error();  // "on any error return the ledger is unchanged": nothing to roll back
    (void)zkr_ledger_release(l, cp);
    set_error("%s", why.c_str());
    *consumed = 0;
    return rc;
  }
  clk.mark(op->ms[0]);
  if (nb == 0) return zkr_ledger_release(l, cp);  // nothing was applied

  // from here on the ledger is ahead of what has been proved: every failure goes through undo()
  const void *const *wit = op->ptrs;
  if (int rc = zkr_rollup_witness_batch_from_device(op->batch, op->depth, op->d_inputs, op->n_public - 1, nb, op->d_wit, op->device, st)) return undo(op, cp, rc);
  clk.mark(op->ms[1]);
  if (op->cs) {
    int ok = 0;
    if (int rc = zkr_r1cs_check_device(op->cs, wit, nb, st, nullptr, &ok)) return undo(op, cp, rc);
    if (!ok) return undo(op, cp, ZKR_ERR_UNSATISFIED);  // the message names the witness and the constraint
    clk.mark(op->ms[2]);
  }
  if (int rc = zkr_prove_batch_device(op->key, wit, nb, r32s, s32s, st, proofs_out)) return undo(op, cp, rc);
  clk.mark(op->ms[3]);
  if (op->vk) {
    std::string verdicts(nb, '\0');
    int all = 0;
    if (int rc = zkr_verify_each_device(op->vk, proofs_out, wit, nb, st, (uint8_t *)&verdicts[0], &all)) return undo(op, cp, rc);
    if (!all) {
      size_t b = 0;
      while (b < nb && !verdicts[b]) b++;
      set_error("batch %zu: proof rejected by the verifying key (verdict %d)", b, b < nb ? (int)(uint8_t)verdicts[b] : -1);
      return undo(op, cp, ZKR_ERR_BAD_KEY);
    }
    clk.mark(op->ms[4]);
  }
  // the public signals: words 1..nPublic of every witness, one strided copy
  const size_t row = (size_t)op->n_public * 32;
  hipError_t e = hipMemcpy2DAsync(publics_out, row, (const uint8_t *)op->d_wit + 32, op->wit_bytes(), row, nb, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    set_error("reading the public signals out failed: %s", hipGetErrorString(e));
    return undo(op, cp, ZKR_ERR_HIP);
  }
  clk.mark(op->ms[5]);
  if (int rc = zkr_ledger_release(l, cp)) return rc;
  *n_batches = nb;
  return ZKR_OK;
}

}  // extern "C"
