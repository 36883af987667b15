// zkr_sequencer.hip -- the operator's ledger on the GPU: a queue of signed transactions in, a status per transaction and the
// input signals of every whole batch out, in device memory, laid out as zkr_rollup_witness_batch_device takes them.
// Replaces the per-transaction host loop of /root/reference/operator/src/routes/send.ts:72-135 (account, balance, fee and nonce
// checks, `verify(formatTx(tx), signature, publicKey)`) and the two leaf moves per transaction of
// operator/src/utils/merkletree.ts:44-83 / operator/src/routes/pubsub.ts:19-66.
//
//   a  signatures     one thread per transaction: S * BASE8 - h * (8A) as ONE projective double-and-add chain over a four-entry
//                     table, compared with R8 by cross-multiplication (no inversion, no signal store: this is not the witness
//                     program of rollup_witness.hpp, which proves the same equation signal by signal)
//   b  ledger pass    on the host (sequencer_plan.cpp): the rules, the 256-bit balance arithmetic, the look-up tables
//   c  leaf hashes    one launch, 2T hashes of four elements
//   d  tree levels    one launch per level, 2T independent hashes each: val[l+1][u] = H(ordered(val[l][u], sib[l][u]))
//   e  assembly       one kernel writes the input signals, a second one the touched nodes' last versions into the ledger's tree
// The field is field.hpp's 8 x 32 limbs throughout, as in the other cold-side kernels; the group law is rollup_witness.hpp's
// (bj_add, bj_dbl, bj_on_curve), the hashes are mimc_device.hpp's (mimc_hash_std, mimc_hash_pair).  Steps c, d and the store are
// the ledger's ONE storing path, stage_updates and store_updates (ledger_internal.hpp): zkr_ledger_sequence, replay() and
// ledger_apply_updates differ in what they derive between the two steps and in the counters they move afterwards.
//
// And the opposite direction: zkr_ledger_replay applies the public signals of published batches to the ledger as
// RollUp.sol:81-161 applies them -- steps a (when asked), b (replay_plan: the contract's arithmetic, none of the operator's
// policy), c, d as above, then replay_compare_kernel, the twin of the assembly, which derives every signal the same way and
// compares it with the claimed one, and the store of the batches in front of the first refused one.
//
// And keeping that state (the host side is ledger_state.cpp / .hpp): read-out of the records and of the stored tree,
// the ZKRLEDG1 snapshot whose restore rebuilds the tree in bulk and compares the root, checkpoints -- a journal of every node a
// storing call is about to overwrite, undone call by call -- and the audit of the stored tree against the records.
#include <stdio.h>
#include <chrono>
#include <memory>
#include <mutex>
#include <vector>
#include "zkr_internal.hpp"
#include "rollup_witness.hpp"
#include "mimc_device.hpp"
#include "sequencer_plan.hpp"
#include "ledger_state.hpp"
#include "ledger_internal.hpp"

namespace zkr {
void rollup_device_constants(Fr *a, Fr *d, uint32_t suborder_m1[8], Fr *b8x253, Fr *b8y253);  // rollup.cpp
int rollup_check_geometry(uint32_t batch, uint32_t depth);

// ------------------------------------------------------------------------------------------------ a. signatures
struct SigConsts {  // the group law itself is rollup_witness.hpp's (bj_add, bj_dbl, bj_on_curve)
  Fr a, d, b8x, b8y;     // Montgomery
  uint32_t suborder[8];  // eddsa.circom:32 (+ 1)
};
// standard form -> Montgomery; false when the words are not below r
__device__ __forceinline__ bool seq_read(const Fr *p, Fr &out) {
  Fr a = *p;
  out = to_mont(a);
  return words_below(a.v, FrParams::P);
}
// the top bit of a 256-bit number, which then moves up by one: a scalar's bits from the top without an indexed register array
__device__ __forceinline__ uint32_t seq_take_top_bit(uint32_t (&w)[8]) {
  const uint32_t b = w[7] >> 31;
#pragma unroll
  for (int i = 7; i > 0; i--) w[i] = (w[i] << 1) | (w[i - 1] >> 31);
  w[0] <<= 1;
  return b;
}
// entry `sel` of four, by masks: the entries stay in registers (a chain of selects becomes an indexed table in scratch)
__device__ __forceinline__ Fr seq_pick(uint32_t sel, const Fr &e0, const Fr &e1, const Fr &e2, const Fr &e3) {
  const uint32_t m0 = 0u - (uint32_t)(sel == 0), m1 = 0u - (uint32_t)(sel == 1), m2 = 0u - (uint32_t)(sel == 2), m3 = 0u - (uint32_t)(sel == 3);
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (e0.v[i] & m0) | (e1.v[i] & m1) | (e2.v[i] & m2) | (e3.v[i] & m3);
  return r;
}

// verdicts[t] = 1 when signature t verifies: R8 and A on the curve, S below the subgroup order, every word below r, and
// S * BASE8 == R8 + h * (8A) with h = multiHash(R8x, R8y, Ax, Ay, multiHash(message)) -- circomlib's verifyMiMCSponge
// (crypto.ts:170-177), the answer of zkr_eddsa_verify.  strict: also refuse a key whose order divides 8 (4A has x = 0), which
// the circuit refuses (eddsa.circom's patched verifier, ST_SMALL_ORDER in rollup_witness.hpp).
// msgs / sigs / pubs: standard form; message elements of any size are taken mod r.  Message and signature t stand at
// (t / group) * group_stride + (t % group) * stride; group 0 is a plain array, t * stride.  The txData rows of
// published batches lie `batch` to a group, one group per batch's signals (zkr_ledger_replay).
static __global__ __launch_bounds__(64) void seq_verify_kernel(const Fr *msgs, size_t msg_stride, uint32_t arity, const Fr *sigs, size_t sig_stride, const Fr *pubs,
                                                               size_t n, uint32_t group, size_t group_stride, SigConsts k, uint32_t strict, uint8_t *verdicts) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  verdicts[t] = 0;
  if (group) msgs += (t / group) * group_stride + (t % group) * msg_stride, sigs += (t / group) * group_stride + (t % group) * sig_stride;
  else msgs += t * msg_stride, sigs += t * sig_stride;
  Fr r8x, r8y, S, ax, ay;
  bool ok = seq_read(sigs, r8x);
  ok = seq_read(sigs + 1, r8y) && ok;
  ok = seq_read(sigs + 2, S) && ok;
  ok = seq_read(pubs + 2 * t, ax) && ok;
  ok = seq_read(pubs + 2 * t + 1, ay) && ok;
  uint32_t sw[8], hw[8];
  {
    const Fr s = sigs[2];
#pragma unroll
    for (int i = 0; i < 8; i++) sw[i] = s.v[i];
  }
  ok = ok && words_below(sw, k.suborder);
  ok = ok && bj_on_curve(k.a, k.d, r8x, r8y) && bj_on_curve(k.a, k.d, ax, ay);
  if (!ok) return;
  {  // h = multiHash(R8x, R8y, Ax, Ay, multiHash(message)): the outer hash's elements are Montgomery already
    const Fr m = mimc_hash_std(msgs, arity);
    Fr r = Fr::zero(), c = Fr::zero();
    mimc_absorb(r, c, r8x);
    mimc_absorb(r, c, r8y);
    mimc_absorb(r, c, ax);
    mimc_absorb(r, c, ay);
    mimc_absorb(r, c, m);
    const Fr h = from_mont(r);
#pragma unroll
    for (int i = 0; i < 8; i++) hw[i] = h.v[i];
  }
  // the table: 0 the identity, 1 BASE8, 2 -(8A), 3 BASE8 - 8A
  const Fr one = Fr::one(), zero = Fr::zero();
  PtD t2{ax, ay, one};
  bool small_order = false;
#pragma unroll 1
  for (int i = 0; i < 3; i++) {
    t2 = bj_dbl(k.a, t2);
    if (i == 1) small_order = t2.x.is_zero();
  }
  if (strict && small_order) return;
  t2.x = neg(t2.x);
  const PtD t1{k.b8x, k.b8y, one};
  const PtD t3 = bj_add(k.a, k.d, t1, t2);
  // S < 2^251 and h < 2^254: 254 steps from bit 253 down
  seq_take_top_bit(sw), seq_take_top_bit(sw);
  seq_take_top_bit(hw), seq_take_top_bit(hw);
  PtD acc{zero, one, one};
#pragma unroll 1
  for (int i = 0; i < 254; i++) {
    acc = bj_dbl(k.a, acc);
    const uint32_t sel = seq_take_top_bit(sw) | (seq_take_top_bit(hw) << 1);
    const PtD q{seq_pick(sel, zero, t1.x, t2.x, t3.x), seq_pick(sel, one, t1.y, t2.y, t3.y), seq_pick(sel, one, t1.z, t2.z, t3.z)};
    acc = bj_add(k.a, k.d, acc, q);  // the identity included: the lanes of a wavefront seldom all skip a step
  }
  // (X : Y : Z) == (R8x, R8y)
  const bool same = !acc.z.is_zero() && acc.x == mul(r8x, acc.z) && acc.y == mul(r8y, acc.z);
  verdicts[t] = same ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ c, d. leaves and levels
// val0[u] = multiHash(record u) (hashBalanceTreeLeaf, operator/src/utils/helpers.ts:80-82); standard form in and out
static __global__ __launch_bounds__(64) void seq_leaf_kernel(const Fr *recs, size_t U, Fr *val0) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  val0[u] = from_mont(mimc_hash_std(recs + 4 * u, 4));
}
// The node above update u's node of level l, as it stands after update u: the hash of that node (val_l[u]) and its sibling, which
// is what the latest earlier update under the sibling left there (val_l[prev_l[u]]) or, without one, the ledger's stored node.
__device__ __forceinline__ Fr seq_sibling(const Fr *val_l, int32_t p, const Fr *tree_l, size_t node) { return p >= 0 ? val_l[p] : tree_l[node ^ 1]; }
static __global__ __launch_bounds__(64) void seq_level_kernel(const Fr *val_l, Fr *val_next, const uint32_t *idx, const int32_t *prev_l, const Fr *tree_l, uint32_t l, size_t U) {
  const size_t u = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const size_t node = (size_t)idx[u] >> l;
  const Fr cur = val_l[u], sib = seq_sibling(val_l, prev_l[u], tree_l, node);
  const bool right = node & 1;
  val_next[u] = mimc_hash_pair(right ? sib : cur, right ? cur : sib);  // both are hashes or stored nodes: below r
}

// ------------------------------------------------------------------------------------------------ e. assembly
// Input signal `rem` of a batch (0 .. batch * (18 + 3 * depth) - 1, circom's order: every input array flattened over the batch,
// rollup_witness.hpp tx_layout, batchprocesstx.circom:13-36) -> its field, the element within the field and the transaction
// within the batch.  The one copy of the width table: 1 8 2 1 1 depth 2 1 1 depth 1 depth.
struct SeqSignal { uint32_t f, j, k; };
__device__ __forceinline__ SeqSignal seq_signal_of(uint32_t rem, uint32_t batch, uint32_t depth) {
  uint32_t f = 0, cnt = 1;
  for (;; f++) {
    cnt = f == 1 ? 8 : (f == 2 || f == 6) ? 2 : (f == 5 || f == 9 || f == 11) ? depth : 1;
    if (rem < batch * cnt) break;
    rem -= batch * cnt;
  }
  return SeqSignal{f, rem % cnt, rem / cnt};
}
// What the ledger derives for element j of field f (any but 1, txData) of applied transaction k.
__device__ __forceinline__ Fr seq_derive(const SeqView &v, uint32_t f, uint32_t j, size_t k) {
  const uint32_t depth = v.depth;
  const size_t us = 2 * k, ur = 2 * k + 1;
  const Fr *root_vals = v.val + (size_t)depth * v.stride;
  if (f == 0) return k == 0 ? v.tree[seq_level_offset(depth, depth)] : root_vals[us - 1];  // balanceTreeRoot
  if (f == 2) return v.old_rec[4 * us + j];                                                 // txSenderPublicKey
  if (f == 3) return v.old_rec[4 * us + 2];                                                 // txSenderBalance
  if (f == 4) return v.old_rec[4 * us + 3];                                                 // txSenderNonce
  if (f == 6) return v.old_rec[4 * ur + j];                                                 // txRecipientPublicKey
  if (f == 7) return v.old_rec[4 * ur + 2];                                                 // txRecipientBalance
  if (f == 8) return v.old_rec[4 * ur + 3];                                                 // txRecipientNonce
  if (f == 10) return root_vals[us];                                                        // intermediateBalanceTreeRoot
  // a path element of level j: the sender's before the transaction (5), the recipient's before it (9: table 1) and after the
  // sender's update (11)
  const size_t u = f == 11 ? ur : us;
  const int32_t p = v.prev[((size_t)(f == 9 ? 1 : 0) * depth + j) * v.U + u];
  const size_t node = (size_t)v.idx[f == 5 ? us : ur] >> j;
  return seq_sibling(v.val + (size_t)j * v.stride, p, v.tree + seq_level_offset(depth, j), node);
}
// One thread per input signal of every batch, in circom's order.
static __global__ __launch_bounds__(256) void seq_assemble_kernel(SeqView v, size_t n_batches, Fr *inputs) {
  const size_t per = (size_t)v.batch * (18 + 3 * v.depth);
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= per * n_batches) return;
  const SeqSignal s = seq_signal_of((uint32_t)(g % per), v.batch, v.depth);
  const size_t k = (g / per) * v.batch + s.k;
  inputs[g] = s.f == 1 ? v.txs[8 * k + s.j] : seq_derive(v, s.f, s.j, k);
}
// The twin of seq_assemble_kernel (zkr_ledger_replay): one thread per PUBLIC signal of every batch -- signal 0 is the batch's
// newBalanceTreeRoot, the root after its last update, then the inputs -- derives it the same way and compares it with the claimed
// one.  first_diff[b] (initialised to 0xFFFFFFFF) ends as the lowest differing signal of batch b; signal 1, the root the batch
// starts from, has a flag of its own (initialised to 0) because its refusal comes first whatever else differs (RollUp.sol:92).
// txData is what everything is derived from and compares equal by construction.
static __global__ __launch_bounds__(256) void replay_compare_kernel(SeqView v, size_t n_batches, const Fr *claimed, uint32_t *first_diff, uint32_t *root_diff) {
  const size_t n_public = 1 + (size_t)v.batch * (18 + 3 * v.depth);
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_public * n_batches) return;
  const size_t bi = g / n_public;
  const uint32_t i = (uint32_t)(g % n_public);
  Fr want;
  if (i == 0) want = v.val[(size_t)v.depth * v.stride + 2 * (bi * v.batch + v.batch - 1) + 1];
  else {
    const SeqSignal s = seq_signal_of(i - 1, v.batch, v.depth);
    if (s.f == 1) return;
    want = seq_derive(v, s.f, s.j, bi * v.batch + s.k);
  }
  if (want == claimed[g]) return;
  if (i == 1) root_diff[bi] = 1;
  else atomicMin(&first_diff[bi], i);
}
// Word 1 + i of witness b -> signal i of batch b, one thread each: the public signals where zkr_verify_each_device reads them.
static __global__ __launch_bounds__(256) void replay_gather_kernel(const Fr *const *witnesses, size_t n_batches, uint32_t n_public, Fr *out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)n_public * n_batches) return;
  out[g] = witnesses[g / n_public][1 + g % n_public];
}
// Thread g of the (depth + 1) x U threads over a stored list -> level l, update u, and whether u holds the LAST version of its
// node of level l (table 2 names it; the root's is the last update's), with that node's offset in the stored tree.  Both are
// facts about the list of U updates that is stored, not about a longer one that was hashed.  The store and the journal decode g
// here and nowhere else: the journal is right exactly when it names the nodes the store writes.
struct SeqWriter { uint32_t l; size_t u, node; bool last; };
__device__ __forceinline__ SeqWriter seq_writer_of(const SeqView &v, size_t g) {
  const uint32_t l = (uint32_t)(g / v.U);
  const size_t u = g % v.U;
  const bool last = l == v.depth ? u == v.U - 1 : v.prev[((size_t)2 * v.depth + l) * v.U + u] != 0;
  return SeqWriter{l, u, last ? seq_level_offset(v.depth, l) + ((size_t)v.idx[u] >> l) : 0, last};
}
// The last version of every touched node goes into the stored tree.
static __global__ __launch_bounds__(256) void seq_store_kernel(SeqView v, Fr *tree) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)v.depth + 1) * v.U) return;
  const SeqWriter w = seq_writer_of(v, g);
  if (w.last) tree[w.node] = v.val[(size_t)w.l * v.stride + w.u];
}
static __global__ __launch_bounds__(256) void seq_fill_kernel(Fr *dst, size_t n, Fr value) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n) dst[g] = value;
}

// ------------------------------------------------------------------------------------------------ keeping the ledger
// The bulk build of a restore: level l (1 .. depth) of the stored tree from level l - 1, for the n = ceil(accounts / 2^l) nodes
// whose subtree holds an account.  A right child past the populated prefix still holds its level's empty-subtree constant.
static __global__ __launch_bounds__(64) void state_build_level_kernel(Fr *tree, uint32_t depth, uint32_t l, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr *below = tree + seq_level_offset(depth, l - 1);
  tree[seq_level_offset(depth, l) + i] = mimc_hash_pair(below[2 * i], below[2 * i + 1]);  // as seq_level_kernel computes it
}
// The journal of a storing call made under a checkpoint: seq_store_kernel's domain and predicate, but instead of writing the new
// value it appends (node offset, the value the tree holds now).  Within one call every node has one last writer, so the entries
// are distinct nodes and their order does not matter; *count starts at 0 and ends as the number of entries, room bounds it.
static __global__ __launch_bounds__(256) void state_journal_kernel(SeqView v, uint32_t *off, Fr *old, uint32_t room, uint32_t *count) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ((size_t)v.depth + 1) * v.U) return;
  const SeqWriter w = seq_writer_of(v, g);
  if (!w.last) return;
  const uint32_t at = atomicAdd(count, 1u);
  if (at < room) off[at] = (uint32_t)w.node, old[at] = v.tree[w.node];
}
// The undo of one journalled call: its old values back where they came from.  n_nodes bounds every offset once more.
static __global__ __launch_bounds__(256) void state_undo_kernel(Fr *tree, size_t n_nodes, const uint32_t *off, const Fr *old, size_t n) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const size_t node = off[g];
  if (node < n_nodes) tree[node] = old[g];
}
// The audit: one thread per node of [node_begin, node_begin + node_count) of the stored tree, every check from stored values
// alone.  Leaf i < accounts equals the leaf hash of record i (only for the records present: recs holds records rec_first ..
// rec_first + rec_count - 1); a node whose subtree lies past the last account equals its level's empty-subtree constant; any
// other inner node equals the hash of its two stored children; and a stored word is below r.  *first_bad (initialised to all
// ones) ends as the lowest (level << 32 | index) that fails.
static __global__ __launch_bounds__(64) void state_audit_kernel(const Fr *tree, uint32_t depth, size_t accounts, const Fr *empty, const Fr *recs, size_t rec_first,
                                                                size_t rec_count, size_t node_begin, size_t node_count, unsigned long long *first_bad) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= node_count) return;
  const size_t g = node_begin + t;
  uint32_t l = 0;
  size_t i = g, width = (size_t)1 << depth;
  while (i >= width) i -= width, width >>= 1, l++;  // g < 2^(depth + 1) - 1: ends with l <= depth
  const Fr have = tree[g];
  bool ok = words_below(have.v, FrParams::P);
  const size_t populated = (accounts + (((size_t)1 << l) - 1)) >> l;
  if (i >= populated) ok = ok && have == empty[l];
  else if (l == 0) {
    if (i < rec_first || i - rec_first >= rec_count) return;  // this launch does not hold the record
    ok = ok && have == from_mont(mimc_hash_std(recs + 4 * (i - rec_first), 4));
  } else {
    const Fr *below = tree + seq_level_offset(depth, l - 1);
    ok = ok && have == mimc_hash_pair(below[2 * i], below[2 * i + 1]);
  }
  if (!ok) atomicMin(first_bad, ((unsigned long long)l << 32) | (unsigned long long)i);
}

// ------------------------------------------------------------------------------------------------ host side
static SigConsts sig_consts() {
  static const SigConsts k = [] {
    SigConsts c;
    std::vector<Fr> tab(2 * 253);
    rollup_device_constants(&c.a, &c.d, c.suborder, tab.data(), tab.data() + 253);
    c.suborder[0] += 1;  // the constant is even (rollup.cpp Bj)
    c.b8x = tab[0], c.b8y = tab[253];
    return c;
  }();
  return k;
}

// Steps c and d for U leaf updates whose records, leaf indices and tables are already in the arena: val[0] from the records, then
// level by level.  Every index the kernels follow was bounded on the host: idx[u] < accounts <= 2^depth, -1 <= prev[l][u] < u.
static int hash_updates(const zkr_ledger *L, size_t U, const Fr *d_new, const uint32_t *d_idx, const int32_t *d_prev, Fr *d_val, hipStream_t s, StageClock &clk, double *ms) {
  seq_leaf_kernel<<<blocks(U, 64), 64, 0, s>>>(d_new, U, d_val);
  ZKR_HIP_CHECK(hipGetLastError());
  clk.mark(ms[2]);
  for (unsigned l = 0; l < L->depth; l++) {
    seq_level_kernel<<<blocks(U, 64), 64, 0, s>>>(d_val + (size_t)l * U, d_val + (size_t)(l + 1) * U, d_idx, d_prev + (size_t)l * U, L->d_tree + seq_level_offset(L->depth, l), l, U);
    ZKR_HIP_CHECK(hipGetLastError());
  }
  clk.mark(ms[3]);
  return ZKR_OK;
}

// ---- keeping the ledger
enum : size_t { STATE_PIECE = (size_t)1 << 20 };  // records go to the device in pieces of at most 2^20: 128 MB of staging

// The journal step of store_updates, run only while a checkpoint is open: between the point where the call's hashes are
// complete (the tree still untouched) and its seq_store_kernel.  v is the view the store will run over, last = its table 2 on
// the host ([depth][v.U]), idx its leaf indices.  The entries land behind the ones in use; *out is the call's host part, which
// store_updates appends to the journal once the store has succeeded -- until then nothing of the journal has moved.  A journal
// that cannot grow is ZKR_ERR_HIP, raised here, before anything is stored.
static int journal_before_store(zkr_ledger *l, const SeqView &v, const int32_t *last, const uint32_t *idx, hipStream_t s, JournalCall *out) {
  const size_t U = v.U, base = l->journal.nodes();
  size_t count = 1;  // the root
  for (size_t i = 0; i < (size_t)v.depth * U; i++) count += last[i] != 0;
  if (base + count > l->jcap) {
    const size_t cap = (base + count) + (base + count) / 2;
    Dev<uint32_t> off;
    Dev<Fr> old;
    if (off.alloc(cap) || old.alloc(cap)) {
      set_error("out of device memory for a checkpoint journal of %zu nodes", cap);
      return ZKR_ERR_HIP;
    }
    hipError_t e = base ? hipMemcpy(off, l->d_joff, base * 4, hipMemcpyDeviceToDevice) : hipSuccess;
    if (e == hipSuccess && base) e = hipMemcpy(old, l->d_jold, base * 32, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { set_error("moving the checkpoint journal failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
    l->d_joff = std::move(off), l->d_jold = std::move(old), l->jcap = cap;
  }
  if (!l->d_jcount)
    if (int rc = l->d_jcount.alloc(1)) return rc;
  uint32_t written = 0;
  ZKR_HIP_CHECK(hipMemsetAsync(l->d_jcount, 0, 4, s));
  state_journal_kernel<<<blocks(((size_t)v.depth + 1) * U, 256), 256, 0, s>>>(v, l->d_joff + base, l->d_jold + base, (uint32_t)count, l->d_jcount);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpyAsync(&written, l->d_jcount, 4, hipMemcpyDeviceToHost, s));
  ZKR_HIP_CHECK(hipStreamSynchronize(s));
  if (written != count) { set_error("internal: the journal holds %u nodes of a call whose tables name %zu", written, count); return ZKR_ERR_HIP; }
  *out = l->journal.record_call(idx, U, l->records, l->accounts, l->applied, l->batches, count);
  if (l->book) {  // what a rollback puts back beside the tree
    out->has_book = true, out->nullifiers_before = l->book->null_count;
    memcpy(out->fees_before, l->book->fees.w, 32);
  }
  return ZKR_OK;
}

// ---- the one storing path: stage_updates, whatever the caller derives from the hashes, store_updates, the caller's counters
size_t update_arena_bytes(size_t U_max, unsigned depth, bool with_old) {  // what stage_updates takes, piece by piece
  return (with_old ? 2 : 1) * DevArena::padded(U_max * 128) + DevArena::padded(((size_t)depth + 1) * U_max * 32) + DevArena::padded(U_max * 4) +
         DevArena::padded(3 * (size_t)depth * U_max * 4);
}
int stage_updates(zkr_ledger *l, const UpdateList &in, size_t accounts, bool check_tables, hipStream_t s, StageClock &clk, double *ms, StagedUpdates *out) {
  const size_t U = in.U, depth = l->depth;
  // every index the kernels follow, once more in one place: a scan without a branch, then the first offender for the message
  size_t bad = 0, u = 0;
  for (size_t i = 0; i < U; i++) bad |= in.idx[i] >= accounts;
  if (bad) {
    while (in.idx[u] < accounts) u++;
    set_error("internal: update %zu names leaf %u of %zu", u, in.idx[u], accounts);
    return ZKR_ERR_ARG;
  }
  for (size_t row = 0; check_tables && row < 2 * depth; row++) {
    const int32_t *p = in.prev + row * U;
    for (size_t i = 0; i < U; i++) bad |= (p[i] < -1) | (p[i] >= (int32_t)i);
    if (!bad) continue;
    while (p[u] >= -1 && p[u] < (int32_t)u) u++;
    set_error("internal: look-up table entry %zu out of range", row * U + u);
    return ZKR_ERR_ARG;
  }
  StagedUpdates d;
  d.U = U;
  d.d_old = in.old_rec ? l->arena.take<Fr>(U * 4) : nullptr, d.d_new = l->arena.take<Fr>(U * 4);
  d.d_val = l->arena.take<Fr>((depth + 1) * U);
  d.d_idx = l->arena.take<uint32_t>(U);
  d.d_prev = l->arena.take<int32_t>(3 * depth * U);
  if (in.old_rec) ZKR_HIP_CHECK(hipMemcpyAsync(d.d_old, in.old_rec, U * 128, hipMemcpyHostToDevice, s));
  ZKR_HIP_CHECK(hipMemcpyAsync(d.d_new, in.new_rec, U * 128, hipMemcpyHostToDevice, s));
  ZKR_HIP_CHECK(hipMemcpyAsync(d.d_idx, in.idx, U * 4, hipMemcpyHostToDevice, s));
  ZKR_HIP_CHECK(hipMemcpyAsync(d.d_prev, in.prev, 3 * depth * U * 4, hipMemcpyHostToDevice, s));
  *out = d;
  return hash_updates(l, U, d.d_new, d.d_idx, d.d_prev, d.d_val, s, clk, ms);
}
int store_updates(zkr_ledger *l, const SeqView &v, const int32_t *last, const uint32_t *idx, const uint8_t *new_rec, hipStream_t s, StageClock &clk, double &slot) {
  ZKR_HIP_CHECK(hipStreamSynchronize(s));  // the tree is untouched up to here: a failure above leaves the ledger as it was
  JournalCall jc;
  const bool journalled = l->journal.open();  // the journal follows the list that is stored, as the store does
  int rc;
  if (journalled && (rc = journal_before_store(l, v, last, idx, s, &jc))) return rc;
  seq_store_kernel<<<blocks(((size_t)v.depth + 1) * v.U, 256), 256, 0, s>>>(v, l->d_tree);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipStreamSynchronize(s));
  if (journalled) l->journal.calls.push_back(std::move(jc));
  clk.mark(slot);
  for (size_t u = 0; u < v.U; u++) memcpy(l->records.data() + (size_t)idx[u] * 128, new_rec + u * 128, 128);  // the records move last
  return ZKR_OK;
}
int ledger_apply_updates(zkr_ledger *l, const uint32_t *indices, const uint8_t *records, size_t n, size_t accounts) {
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  const unsigned depth = l->depth;
  std::vector<uint32_t> idx(indices, indices + n);
  std::vector<int32_t> prev(3 * (size_t)depth * n);
  seq_tables(depth, idx, nullptr, accounts, prev.data());
  int rc = l->arena.reserve(update_arena_bytes(n, depth, false));
  if (rc) return rc;
  hipStream_t s = nullptr;
  StageClock clk(s);
  clk.on = false;
  double unused[5];
  StagedUpdates st;
  if ((rc = stage_updates(l, UpdateList{n, indices, records, nullptr, prev.data()}, accounts, false, s, clk, unused, &st))) return rc;
  l->records.resize(accounts * 128);  // room for the accounts the list adds; they count once l->accounts moves
  if ((rc = store_updates(l, st.view(l, nullptr, 1, n), prev.data() + 2 * (size_t)depth * n, indices, records, s, clk, unused[4]))) {
    l->records.resize(l->accounts * 128);
    return rc;
  }
  l->accounts = accounts;
  return ZKR_OK;
}

// Step a's keys: the senders' stored keys beside their transactions.  Row t (eight words, `from` first) stands where
// seq_verify_kernel finds it: group 0 is a plain array, else (t / group) * group_stride + (t % group) * 8 words behind `rows`.
// A sender that is no account gets the all-zero key, which is on no curve.
static std::vector<uint8_t> sender_keys(const zkr_ledger *l, const uint8_t *rows, size_t n_txs, uint32_t group, size_t group_stride) {
  std::vector<uint8_t> keys(n_txs * 64, 0);
  for (size_t t = 0; t < n_txs; t++) {
    const Int256 from = int256_load(rows + (group ? (t / group) * group_stride + (t % group) * 8 : t * 8) * 32);
    if (!(from.w[1] | from.w[2] | from.w[3]) && from.w[0] < l->accounts) memcpy(&keys[t * 64], l->records.data() + (size_t)from.w[0] * 128, 64);
  }
  return keys;
}
// The old and new records of a plan's first U updates as the device takes them: 128 B each, standard form.
static void pack_records(const SeqPlan &plan, size_t U, std::vector<uint8_t> &h_old, std::vector<uint8_t> &h_new) {
  h_new.resize(U * 128), h_old.resize(U * 128);
  for (size_t u = 0; u < U; u++)
    for (int j = 0; j < 4; j++) int256_store(&h_old[u * 128 + 32 * j], plan.old_rec[u].f[j]), int256_store(&h_new[u * 128 + 32 * j], plan.new_rec[u].f[j]);
}
}  // namespace zkr

using namespace zkr;

namespace {

// The bulk build of a restore: L->records and L->accounts are set and checked, the tree is the empty one of zkr_ledger_new.
// Leaf hashes straight into level 0, then one launch per level over the nodes whose subtree holds an account: no tables, no
// value buffer, fewer than 2 * accounts + depth hashes.  Default stream; returns synchronised.
int bulk_build(zkr_ledger *L) {
  const size_t accounts = L->accounts;
  if (!accounts) return ZKR_OK;
  const size_t piece = accounts < STATE_PIECE ? accounts : (size_t)STATE_PIECE;
  int rc = L->arena.reserve(DevArena::padded(piece * 128));
  if (rc) return rc;
  Fr *d_stage = L->arena.take<Fr>(piece * 4);
  for (size_t first = 0; first < accounts; first += piece) {
    const size_t n = accounts - first < piece ? accounts - first : piece;
    ZKR_HIP_CHECK(hipMemcpy(d_stage, L->records.data() + first * 128, n * 128, hipMemcpyHostToDevice));
    seq_leaf_kernel<<<blocks(n, 64), 64>>>(d_stage, n, L->d_tree + first);
    ZKR_HIP_CHECK(hipGetLastError());
  }
  for (unsigned lv = 1; lv <= L->depth; lv++) {
    const size_t n = (accounts + (((size_t)1 << lv) - 1)) >> lv;  // <= 2^(depth - lv), the level's width
    state_build_level_kernel<<<blocks(n, 64), 64>>>(L->d_tree, L->depth, lv, n);
    ZKR_HIP_CHECK(hipGetLastError());
  }
  ZKR_HIP_CHECK(hipDeviceSynchronize());
  return ZKR_OK;
}

void hex_be(const uint8_t le[32], char out[67]) {
  out[0] = '0', out[1] = 'x';
  for (int i = 0; i < 32; i++) snprintf(out + 2 + 2 * i, 3, "%02x", le[31 - i]);
}

// zkr_ledger_replay and zkr_ledger_replay_device: exactly one of publics (host) and d_witnesses (a host array of device pointers)
// is set.  Stage times, when asked for: 0 the signals' way to both sides and the signatures, 1 the host pass, 2 leaf hashes,
// 3 tree levels, 4 comparison and store.
int replay(zkr_ledger *l, const uint8_t *publics, const void *const *d_witnesses, size_t n_batches, uint32_t batch, const uint8_t *proof_verdicts,
           uint32_t flags, uint8_t *verdicts, uint32_t *where, size_t *applied, void *stream) {
  if (applied) *applied = 0;
  if (!l || !applied || (n_batches && ((!publics && !d_witnesses) || !verdicts || !where))) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (flags & ~ZKR_REPLAY_SIGNATURES) { set_error("unknown replay flags %#x", flags); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  const unsigned depth = l->depth;
  int rc = rollup_check_geometry(batch, depth);
  if (rc) return rc;
  if (n_batches > ((size_t)1 << 22) / batch) { set_error("more than 2^22 transactions in one run of batches"); return ZKR_ERR_ARG; }
  for (size_t b = 0; d_witnesses && b < n_batches; b++)
    if (!d_witnesses[b]) { set_error("witness %zu is a null pointer", b); return ZKR_ERR_ARG; }
  if (n_batches == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  hipStream_t s = (hipStream_t)stream;
  double ms[5] = {0, 0, 0, 0, 0};
  StageClock clk(s);
  const bool with_sigs = flags & ZKR_REPLAY_SIGNATURES;
  const size_t n_public = 1 + (size_t)batch * (18 + 3 * (size_t)depth), n_txs = n_batches * batch, U_max = 2 * n_txs;
  rc = l->arena.reserve(DevArena::padded(n_batches * n_public * 32) + DevArena::padded(n_batches * sizeof(void *)) + DevArena::padded(n_txs * 64) +
                        DevArena::padded(n_txs) + DevArena::padded(2 * n_batches * 4) + update_arena_bytes(U_max, depth, true));
  if (rc) return rc;
  Fr *d_claimed = l->arena.take<Fr>(n_batches * n_public);
  const Fr **d_ptrs = l->arena.take<const Fr *>(n_batches);
  Fr *d_keys = l->arena.take<Fr>(n_txs * 2);
  uint8_t *d_sig = l->arena.take<uint8_t>(n_txs);
  uint32_t *d_diff = l->arena.take<uint32_t>(2 * n_batches);

  // the claimed signals on both sides
  std::vector<uint8_t> gathered;
  if (publics) ZKR_HIP_CHECK(hipMemcpyAsync(d_claimed, publics, n_batches * n_public * 32, hipMemcpyHostToDevice, s));
  else {
    gathered.resize(n_batches * n_public * 32);
    ZKR_HIP_CHECK(hipMemcpyAsync(d_ptrs, d_witnesses, n_batches * sizeof(void *), hipMemcpyHostToDevice, s));
    replay_gather_kernel<<<blocks(n_batches * n_public, 256), 256, 0, s>>>(d_ptrs, n_batches, (uint32_t)n_public, d_claimed);
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpyAsync(gathered.data(), d_claimed, gathered.size(), hipMemcpyDeviceToHost, s));
    ZKR_HIP_CHECK(hipStreamSynchronize(s));
    publics = gathered.data();
  }

  // a. signatures over the txData rows where they lie, under the senders' stored keys; a sender that is no account gets a key
  // that is on no curve (its batch is refused with code 1 before the signature is looked at)
  std::vector<uint8_t> sig_ok(n_txs, 1);
  if (with_sigs) {
    const std::vector<uint8_t> keys = sender_keys(l, publics + (1 + (size_t)batch) * 32, n_txs, batch, n_public);
    ZKR_HIP_CHECK(hipMemcpyAsync(d_keys, keys.data(), n_txs * 64, hipMemcpyHostToDevice, s));
    const Fr *rows = d_claimed + 1 + batch;
    seq_verify_kernel<<<blocks(n_txs, 64), 64, 0, s>>>(rows, 8, 5, rows + 5, 8, d_keys, n_txs, batch, n_public, sig_consts(), 1, d_sig);
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpyAsync(sig_ok.data(), d_sig, n_txs, hipMemcpyDeviceToHost, s));
    ZKR_HIP_CHECK(hipStreamSynchronize(s));
  }
  clk.mark(ms[0]);

  // b. the pass: every batch up to the first that cannot be applied
  SeqPlan plan;
  const char *why = "";
  size_t planned = 0;
  uint32_t where1 = 0;
  if (replay_plan(depth, l->records.data(), l->accounts, publics, n_batches, batch, plan, &planned, &where1, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  clk.mark(ms[1]);
  const size_t U = 2 * planned * batch;
  std::vector<uint8_t> h_new;
  std::vector<uint32_t> diff(2 * n_batches, 0);
  StagedUpdates st;
  if (U) {
    std::vector<uint8_t> h_old;  // only the comparison reads them
    pack_records(plan, U, h_old, h_new);
    ZKR_HIP_CHECK(hipMemsetAsync(d_diff, 0xFF, planned * 4, s));
    ZKR_HIP_CHECK(hipMemsetAsync(d_diff + n_batches, 0, planned * 4, s));
    if ((rc = stage_updates(l, UpdateList{U, plan.idx.data(), h_new.data(), h_old.data(), plan.prev.data()}, l->accounts, true, s, clk, ms, &st))) return rc;
    replay_compare_kernel<<<blocks(planned * n_public, 256), 256, 0, s>>>(st.view(l, nullptr, batch, U), planned, d_claimed, d_diff, d_diff + n_batches);
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpyAsync(diff.data(), d_diff, planned * 4, hipMemcpyDeviceToHost, s));
    ZKR_HIP_CHECK(hipMemcpyAsync(diff.data() + n_batches, d_diff + n_batches, planned * 4, hipMemcpyDeviceToHost, s));
    ZKR_HIP_CHECK(hipStreamSynchronize(s));  // the tree is untouched up to here: a failure above leaves the ledger as it was
  }

  // the first refused batch B, by the precedence of include/zkr.h
  size_t B = planned;
  uint8_t code = planned < n_batches ? 1 : 0;
  uint32_t at = where1;
  for (size_t b = 0; b < planned; b++) {
    uint8_t c = 0;
    uint32_t w = 0;
    if (diff[n_batches + b]) c = 2, w = 1;
    else if (proof_verdicts && proof_verdicts[b]) c = 3;
    else {
      for (uint32_t k = 0; k < batch && !c; k++)
        if (!sig_ok[b * batch + k]) c = 5, w = k;
      if (!c && diff[b] != 0xFFFFFFFFu) c = 4, w = diff[b];
    }
    if (c) { B = b, code = c, at = w; break; }
  }

  // e. only the updates of batches 0 .. B - 1 go into the tree; the records move last
  const size_t Ub = 2 * B * batch;
  if (Ub) {
    std::vector<int32_t> prev;
    if (Ub < U) {  // "holds the last version of its node" is a fact about the stored list: the tables of the prefix
      std::vector<uint32_t> idx(plan.idx.begin(), plan.idx.begin() + Ub);
      prev.resize(3 * (size_t)depth * Ub);
      seq_tables(depth, idx, nullptr, l->accounts, prev.data());
      ZKR_HIP_CHECK(hipMemcpyAsync(st.d_prev, prev.data(), prev.size() * 4, hipMemcpyHostToDevice, s));  // the step below waits for it
    }
    // val keeps the rows of the hashed list: the view's stride stays U
    if ((rc = store_updates(l, st.view(l, nullptr, batch, Ub), (Ub < U ? prev.data() : plan.prev.data()) + 2 * (size_t)depth * Ub, plan.idx.data(), h_new.data(), s, clk, ms[4]))) return rc;
    l->applied += B * batch, l->batches += B;
    if (l->book)  // accuredFees += fee (RollUp.sol:139): signal 1 + batch + 8k + 3 of every applied batch
      for (size_t t = 0; t < B * batch; t++) l->book->fees = int256_add(l->book->fees, int256_load(publics + ((t / batch) * n_public + 1 + batch + 8 * (t % batch) + 3) * 32));
  }
  double tail = 0;  // a replay's slot 4 runs to here, as it always did: the records' copy and the fees are in it
  clk.mark(tail);
  ms[4] += tail;
  for (size_t b = 0; b < n_batches; b++) {
    verdicts[b] = b < B ? 0 : b == B ? code : SEQ_NOT_REACHED;
    where[b] = b == B ? at : 0;
  }
  *applied = B;
  if (clk.on) memcpy(l->stage_ms, ms, sizeof ms);
  return ZKR_OK;
}
}  // namespace

extern "C" {

int zkr_ledger_new(unsigned depth, int device, zkr_ledger **out) {
  if (!out) { set_error("null argument"); return ZKR_ERR_ARG; }
  *out = nullptr;
  if (depth < 1 || depth > 24) { set_error("ledger depth %u out of range (1..24)", depth); return ZKR_ERR_ARG; }
  int rc = need_device(device, "the ledger");
  if (rc) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  if ((rc = upload_mimc_constants(device))) return rc;
  std::unique_ptr<zkr_ledger> L(new zkr_ledger);
  L->depth = depth, L->device = device;
  const size_t total = ((size_t)2 << depth) - 1;
  if (L->d_tree.alloc(total)) { set_error("out of device memory for a tree of depth %u", depth); return ZKR_ERR_HIP; }
  uint8_t z[64] = {0};  // the empty tree: every node of a level is the hash of two empty nodes below (merkletree.ts:44-60)
  hipError_t e = hipSuccess;
  for (unsigned l = 0; l <= depth && e == hipSuccess; l++) {
    Fr v;
    memcpy(v.v, z, 32);
    L->empty.insert(L->empty.end(), z, z + 32);
    const size_t width = (size_t)1 << (depth - l);
    seq_fill_kernel<<<blocks(width, 256), 256>>>(L->d_tree + seq_level_offset(depth, l), width, v);
    e = hipGetLastError();
    memcpy(z + 32, z, 32);
    zkr_mimcsponge_multihash(z, 2, z);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("ledger tree fill failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  *out = L.release();
  return ZKR_OK;
}

void zkr_ledger_free(zkr_ledger *l) {
  if (!l) return;
  (void)hipSetDevice(l->device);
  delete l;  // the tree, the arena, the journal and the book's tables go with their owners
}

int zkr_ledger_info(const zkr_ledger *l, uint64_t out[4]) {
  if (!l || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  out[0] = l->depth, out[1] = l->accounts, out[2] = l->applied, out[3] = l->batches;
  return ZKR_OK;
}

int zkr_ledger_stage_times(const zkr_ledger *l, double ms[5]) {
  if (!l || !ms) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  for (int i = 0; i < 5; i++) ms[i] = l->stage_ms[i];
  return ZKR_OK;
}

int zkr_ledger_root(const zkr_ledger *l, uint8_t root[32]) {
  if (!l || !root) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  ZKR_HIP_CHECK(hipMemcpy(root, l->d_tree + seq_level_offset(l->depth, l->depth), 32, hipMemcpyDeviceToHost));
  return ZKR_OK;
}

int zkr_ledger_account(const zkr_ledger *l, uint32_t index, uint8_t record[128], uint8_t *path) {
  if (!l || !record) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  if (index >= l->accounts) { set_error("account %u of %zu", index, l->accounts); return ZKR_ERR_ARG; }
  memcpy(record, l->records.data() + (size_t)index * 128, 128);
  if (!path) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  for (unsigned lv = 0; lv < l->depth; lv++)  // getUpdatePath(index).pathElements: the sibling per level, leaf level first
    ZKR_HIP_CHECK(hipMemcpy(path + 32 * lv, l->d_tree + seq_level_offset(l->depth, lv) + (((size_t)index >> lv) ^ 1), 32, hipMemcpyDeviceToHost));
  return ZKR_OK;
}

int zkr_ledger_deposit(zkr_ledger *l, const uint32_t *indices, const uint8_t *records, size_t n) {
  if (!l || (n && (!indices || !records))) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (n == 0) return ZKR_OK;
  if (n > ((size_t)1 << 24)) { set_error("more than 2^24 records in one deposit"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  size_t accounts = l->accounts;
  for (size_t i = 0; i < n; i++) {
    if (indices[i] > accounts) { set_error("deposit %zu: index %u is out of sync with the ledger's %zu accounts (pubsub.ts:37-41)", i, indices[i], accounts); return ZKR_ERR_ARG; }
    if (indices[i] == accounts) {
      if (accounts == ((size_t)1 << l->depth)) { set_error("deposit %zu: the tree of depth %u is full", i, l->depth); return ZKR_ERR_ARG; }
      accounts++;
    }
    for (int j = 0; j < 4; j++) {
      const Int256 v = int256_load(records + i * 128 + 32 * j);
      if (!int256_below_r(v) || (j >= 2 && !int256_below_2_250(v))) {
        set_error("deposit %zu: element %d is not below r, or a balance / nonce does not fit the circuit's 250 bits", i, j);
        return ZKR_ERR_ARG;
      }
    }
  }
  if (l->book)  // a key written where another one stood, or a new account: the key table no longer says what the records say
    for (size_t i = 0; i < n && !l->book->keys_stale; i++)
      if (indices[i] >= l->accounts || memcmp(l->records.data() + (size_t)indices[i] * 128, records + i * 128, 64)) l->book->keys_stale = true;
  return ledger_apply_updates(l, indices, records, n, accounts);
}

int zkr_eddsa_verify_batch(const uint8_t *msgs, unsigned arity, const uint8_t *sigs, const uint8_t *pubs, size_t n, uint8_t *verdicts, int device) {
  if (n && (!msgs || !sigs || !pubs || !verdicts)) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (arity < 1 || arity > 64) { set_error("message arity %u out of range (1..64)", arity); return ZKR_ERR_ARG; }
  if (n > ((size_t)1 << 24)) { set_error("more than 2^24 signatures in one call"); return ZKR_ERR_ARG; }
  int rc = need_device(device, "the batch signature check (zkr_eddsa_verify is the host call)");
  if (rc) return rc;
  if (n == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(device));
  if ((rc = upload_mimc_constants(device))) return rc;
  const size_t mb = DevArena::padded(n * arity * 32), sb = DevArena::padded(n * 96), pb = DevArena::padded(n * 64);
  Dev<char> d;
  if ((rc = d.alloc(mb + sb + pb + n))) return rc;
  Fr *d_msgs = (Fr *)d, *d_sigs = (Fr *)(d + mb), *d_pubs = (Fr *)(d + mb + sb);
  uint8_t *d_v = (uint8_t *)(d + mb + sb + pb);
  hipError_t e = hipMemcpy(d_msgs, msgs, n * arity * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_sigs, sigs, n * 96, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_pubs, pubs, n * 64, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    seq_verify_kernel<<<blocks(n, 64), 64>>>(d_msgs, arity, arity, d_sigs, 3, d_pubs, n, 0, 0, sig_consts(), 0, d_v);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(verdicts, d_v, n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { set_error("batch signature check failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  return ZKR_OK;
}

int zkr_ledger_sequence(zkr_ledger *l, const uint8_t *txs, size_t n_txs, uint32_t batch, uint8_t *status, void *d_inputs, size_t *n_batches, size_t *consumed, void *stream) {
  if (!l || !d_inputs || !n_batches || !consumed || (n_txs && (!txs || !status))) { set_error("null argument"); return ZKR_ERR_ARG; }
  *n_batches = 0, *consumed = 0;
  std::lock_guard<std::mutex> lk(l->mu);
  const unsigned depth = l->depth;
  int rc = rollup_check_geometry(batch, depth);
  if (rc) return rc;
  if (n_txs > ((size_t)1 << 22)) { set_error("more than 2^22 transactions in one queue"); return ZKR_ERR_ARG; }
  if (n_txs == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  hipStream_t s = (hipStream_t)stream;
  double ms[5] = {0, 0, 0, 0, 0};
  StageClock clk(s);

  // a. the senders' stored keys beside their transactions; a sender that is no account gets a key that is on no curve
  const std::vector<uint8_t> keys = sender_keys(l, txs, n_txs, 0, 0);
  std::vector<uint8_t> verdicts(n_txs);
  rc = l->arena.reserve(2 * DevArena::padded(n_txs * 256) + DevArena::padded(n_txs * 64) + DevArena::padded(n_txs) + update_arena_bytes(2 * n_txs, depth, true));
  if (rc) return rc;
  Fr *d_queue = l->arena.take<Fr>(n_txs * 8), *d_keys = l->arena.take<Fr>(n_txs * 2);
  uint8_t *d_verdicts = l->arena.take<uint8_t>(n_txs);
  ZKR_HIP_CHECK(hipMemcpyAsync(d_queue, txs, n_txs * 256, hipMemcpyHostToDevice, s));
  ZKR_HIP_CHECK(hipMemcpyAsync(d_keys, keys.data(), n_txs * 64, hipMemcpyHostToDevice, s));
  seq_verify_kernel<<<blocks(n_txs, 64), 64, 0, s>>>(d_queue, 8, 5, d_queue + 5, 8, d_keys, n_txs, 0, 0, sig_consts(), 1, d_verdicts);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpyAsync(verdicts.data(), d_verdicts, n_txs, hipMemcpyDeviceToHost, s));
  ZKR_HIP_CHECK(hipStreamSynchronize(s));
  clk.mark(ms[0]);

  // b. the pass
  SeqPlan plan;
  const char *why = "";
  if (seq_plan(depth, l->records.data(), l->accounts, txs, n_txs, verdicts.data(), batch, plan, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  clk.mark(ms[1]);
  const size_t T = plan.applied, U = 2 * T;
  if (T) {
    std::vector<uint8_t> h_txs(T * 256), h_old, h_new;
    for (size_t k = 0; k < T; k++) memcpy(&h_txs[k * 256], txs + (size_t)plan.pos[k] * 256, 256);
    pack_records(plan, U, h_old, h_new);
    Fr *d_txs = l->arena.take<Fr>(T * 8);
    ZKR_HIP_CHECK(hipMemcpyAsync(d_txs, h_txs.data(), h_txs.size(), hipMemcpyHostToDevice, s));
    StagedUpdates st;
    if ((rc = stage_updates(l, UpdateList{U, plan.idx.data(), h_new.data(), h_old.data(), plan.prev.data()}, l->accounts, true, s, clk, ms, &st))) return rc;
    const size_t nb = T / batch;
    const SeqView v = st.view(l, d_txs, batch, U);
    seq_assemble_kernel<<<blocks(nb * batch * (18 + 3 * (size_t)depth), 256), 256, 0, s>>>(v, nb, (Fr *)d_inputs);
    ZKR_HIP_CHECK(hipGetLastError());
    if ((rc = store_updates(l, v, plan.prev.data() + 2 * (size_t)depth * U, plan.idx.data(), h_new.data(), s, clk, ms[4]))) return rc;
    l->applied += T, l->batches += nb;
    if (l->book)  // accuredFees += fee (RollUp.sol:139)
      for (size_t k = 0; k < T; k++) l->book->fees = int256_add(l->book->fees, int256_load(&h_txs[k * 256 + 96]));
    *n_batches = nb;
  }
  memcpy(status, plan.status.data(), n_txs);
  *consumed = plan.consumed;
  if (clk.on) memcpy(l->stage_ms, ms, sizeof ms);
  return ZKR_OK;
}

int zkr_ledger_replay(zkr_ledger *l, const void *publics_std, size_t n_batches, uint32_t batch, const uint8_t *proof_verdicts, uint32_t flags,
                      uint8_t *verdicts, uint32_t *where, size_t *applied, void *stream) {
  if (applied) *applied = 0;
  if (n_batches && !publics_std) { set_error("null argument"); return ZKR_ERR_ARG; }
  return replay(l, (const uint8_t *)publics_std, nullptr, n_batches, batch, proof_verdicts, flags, verdicts, where, applied, stream);
}

int zkr_ledger_replay_device(zkr_ledger *l, const void *const *d_witnesses_std, size_t n_batches, uint32_t batch, const uint8_t *proof_verdicts,
                             uint32_t flags, uint8_t *verdicts, uint32_t *where, size_t *applied, void *stream) {
  if (applied) *applied = 0;
  if (n_batches && !d_witnesses_std) { set_error("null argument"); return ZKR_ERR_ARG; }
  return replay(l, nullptr, d_witnesses_std, n_batches, batch, proof_verdicts, flags, verdicts, where, applied, stream);
}

// ------------------------------------------------------------------------------------------------ keeping the ledger
int zkr_ledger_records(const zkr_ledger *l, size_t first, size_t count, uint8_t *out) {
  if (!l || (count && !out)) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  if (first > l->accounts || count > l->accounts - first) { set_error("records %zu .. %zu + %zu of %zu accounts", first, first, count, l->accounts); return ZKR_ERR_ARG; }
  if (count) memcpy(out, l->records.data() + first * 128, count * 128);
  return ZKR_OK;
}

int zkr_ledger_tree(const zkr_ledger *l, const void **dev_ptr, size_t *len) {
  if (!l || !dev_ptr || !len) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  *dev_ptr = l->d_tree, *len = (((size_t)2 << l->depth) - 1) * 32;
  return ZKR_OK;
}

int zkr_ledger_snapshot(const zkr_ledger *l, void **blob, size_t *len) {
  if (blob) *blob = nullptr;
  if (!l || !blob || !len) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  LedgerHeader h;
  h.depth = l->depth, h.accounts = l->accounts, h.applied = l->applied, h.batches = l->batches;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  ZKR_HIP_CHECK(hipMemcpy(h.root, l->d_tree + seq_level_offset(l->depth, l->depth), 32, hipMemcpyDeviceToHost));
  const size_t n = LEDGER_HEADER_BYTES + l->accounts * 128;
  uint8_t *out = (uint8_t *)malloc(n);
  if (!out) { set_error("out of memory for a snapshot of %zu bytes", n); return ZKR_ERR_ARG; }
  if (ledger_header_write(h, out)) { free(out); set_error("the snapshot's tag could not be computed"); return ZKR_ERR_ARG; }
  if (l->accounts) memcpy(out + LEDGER_HEADER_BYTES, l->records.data(), l->accounts * 128);
  *blob = out, *len = n;
  return ZKR_OK;
}

int zkr_ledger_save(const zkr_ledger *l, const char *path) {
  if (!l || !path) { set_error("null argument"); return ZKR_ERR_ARG; }
  void *blob = nullptr;
  size_t len = 0;
  int rc = zkr_ledger_snapshot(l, &blob, &len);
  if (rc) return rc;
  const std::string tmp = std::string(path) + ".tmp";  // either the old file or the new one, never a part of one
  FILE *f = fopen(tmp.c_str(), "wb");
  bool ok = f != nullptr;
  if (f) {
    ok = fwrite(blob, 1, len, f) == len;
    ok = fflush(f) == 0 && ok;
    ok = fclose(f) == 0 && ok;
  }
  free(blob);
  if (ok) ok = rename(tmp.c_str(), path) == 0;
  if (!ok) { remove(tmp.c_str()); set_error("cannot write the ledger snapshot to %s", path); return ZKR_ERR_ARG; }
  return ZKR_OK;
}

int zkr_ledger_restore(const void *blob, size_t len, int device, zkr_ledger **out) {
  if (out) *out = nullptr;
  if (!blob || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  LedgerHeader h;
  char why[200];
  if (ledger_snapshot_parse((const uint8_t *)blob, len, &h, why, sizeof why)) { set_error("%s", why); return ZKR_ERR_ARG; }  // before the device is looked at
  int rc = need_device(device, "restoring a ledger");
  if (rc) return rc;
  zkr_ledger *L = nullptr;
  if ((rc = zkr_ledger_new(h.depth, device, &L))) return rc;
  L->accounts = (size_t)h.accounts;
  L->records.assign((const uint8_t *)blob + LEDGER_HEADER_BYTES, (const uint8_t *)blob + len);
  uint8_t root[32];
  rc = bulk_build(L);
  if (!rc && hipMemcpy(root, L->d_tree + seq_level_offset(L->depth, L->depth), 32, hipMemcpyDeviceToHost) != hipSuccess) {
    set_error("reading the rebuilt root failed");
    rc = ZKR_ERR_HIP;
  }
  if (!rc && memcmp(root, h.root, 32)) {  // the root pins the records: the stored one is not trusted, it is compared
    char want[67], got[67];
    hex_be(h.root, want), hex_be(root, got);
    set_error("ledger snapshot: the records rebuild to root %s, the snapshot says %s", got, want);
    rc = ZKR_ERR_BAD_KEY;
  }
  if (rc) { zkr_ledger_free(L); return rc; }
  L->applied = h.applied, L->batches = h.batches;
  *out = L;
  return ZKR_OK;
}

int zkr_ledger_load_file(const char *path, int device, zkr_ledger **out) {
  if (out) *out = nullptr;
  if (!path || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  FILE *f = fopen(path, "rb");
  if (!f) { set_error("cannot open %s", path); return ZKR_ERR_ARG; }
  std::vector<uint8_t> buf;
  uint8_t chunk[1 << 16];
  size_t n;
  while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
  const bool bad = ferror(f);
  fclose(f);
  if (bad) { set_error("cannot read %s", path); return ZKR_ERR_ARG; }
  return zkr_ledger_restore(buf.data(), buf.size(), device, out);
}

int zkr_ledger_checkpoint(zkr_ledger *l, uint64_t *id) {
  if (!l || !id) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  *id = l->journal.checkpoint();
  return ZKR_OK;
}

int zkr_ledger_release(zkr_ledger *l, uint64_t id) {
  if (!l) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  if (!l->journal.release(id)) { set_error("checkpoint %llu is not open (unknown, released or discarded by a rollback)", (unsigned long long)id); return ZKR_ERR_ARG; }
  return ZKR_OK;
}

int zkr_ledger_rollback(zkr_ledger *l, uint64_t id) {
  if (!l) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  const long keep = l->journal.rollback_keep(id);
  if (keep < 0) { set_error("checkpoint %llu is not open (unknown, released or discarded by a rollback)", (unsigned long long)id); return ZKR_ERR_ARG; }
  const std::vector<JournalCall> &calls = l->journal.calls;
  if (calls.size() > (size_t)keep) {
    ZKR_HIP_CHECK(hipSetDevice(l->device));
    const size_t n_nodes = ((size_t)2 << l->depth) - 1;
    for (size_t c = calls.size(); c-- > (size_t)keep;) {  // call by call, the latest first: two calls may hold the same node
      state_undo_kernel<<<blocks(calls[c].node_count, 256), 256>>>(l->d_tree, n_nodes, l->d_joff + calls[c].node_begin, l->d_jold + calls[c].node_begin, calls[c].node_count);
      ZKR_HIP_CHECK(hipGetLastError());
    }
    ZKR_HIP_CHECK(hipDeviceSynchronize());
    for (size_t c = calls.size(); c-- > (size_t)keep;) {
      LedgerJournal::undo_host(calls[c], l->records, l->accounts, l->applied, l->batches);
      if (l->book && calls[c].has_book) l->book->null_count = calls[c].nullifiers_before, memcpy(l->book->fees.w, calls[c].fees_before, 32);
    }
    if (l->book) l->book->keys_stale = l->book->null_stale = true;  // both tables may name what is gone: rebuilt at the next by-key call
  }
  l->journal.rollback_done(id);
  return ZKR_OK;
}

int zkr_ledger_journal_info(const zkr_ledger *l, uint64_t out[2]) {
  if (!l || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  out[0] = l->journal.markers.size(), out[1] = l->journal.nodes();
  return ZKR_OK;
}

int zkr_ledger_audit(zkr_ledger *l, uint64_t report[2], int *sound) {
  if (sound) *sound = 0;
  if (!l || !report || !sound) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  const unsigned depth = l->depth;
  const size_t accounts = l->accounts, n_nodes = ((size_t)2 << depth) - 1;
  const size_t piece = accounts < STATE_PIECE ? accounts : (size_t)STATE_PIECE;
  int rc = l->arena.reserve(DevArena::padded(piece * 128 + 128) + DevArena::padded(((size_t)depth + 1) * 32) + DevArena::padded(8));
  if (rc) return rc;
  Fr *d_stage = l->arena.take<Fr>(piece * 4 + 4), *d_empty = l->arena.take<Fr>(depth + 1);
  unsigned long long *d_bad = l->arena.take<unsigned long long>(1), bad = ~0ull;
  ZKR_HIP_CHECK(hipMemcpy(d_empty, l->empty.data(), ((size_t)depth + 1) * 32, hipMemcpyHostToDevice));
  ZKR_HIP_CHECK(hipMemset(d_bad, 0xFF, 8));
  if (piece) ZKR_HIP_CHECK(hipMemcpy(d_stage, l->records.data(), piece * 128, hipMemcpyHostToDevice));
  // one launch over every node, with the first piece of records; a ledger of more than 2^20 accounts then has its remaining
  // leaves looked at piece by piece
  state_audit_kernel<<<blocks(n_nodes, 64), 64>>>(l->d_tree, depth, accounts, d_empty, d_stage, 0, piece, 0, n_nodes, d_bad);
  ZKR_HIP_CHECK(hipGetLastError());
  for (size_t first = piece; first < accounts; first += piece) {
    const size_t n = accounts - first < piece ? accounts - first : piece;
    ZKR_HIP_CHECK(hipMemcpy(d_stage, l->records.data() + first * 128, n * 128, hipMemcpyHostToDevice));
    state_audit_kernel<<<blocks(n, 64), 64>>>(l->d_tree, depth, accounts, d_empty, d_stage, first, n, first, n, d_bad);
    ZKR_HIP_CHECK(hipGetLastError());
  }
  ZKR_HIP_CHECK(hipMemcpy(&bad, d_bad, 8, hipMemcpyDeviceToHost));
  ZKR_HIP_CHECK(hipDeviceSynchronize());
  report[0] = report[1] = 0;
  if (bad == ~0ull) { *sound = 1; return ZKR_OK; }
  report[0] = bad >> 32, report[1] = bad & 0xFFFFFFFFull;
  set_error("ledger audit: node %llu of level %llu is not what the records and the nodes below it make it", (unsigned long long)report[1], (unsigned long long)report[0]);
  return ZKR_OK;
}

}  // extern "C"
