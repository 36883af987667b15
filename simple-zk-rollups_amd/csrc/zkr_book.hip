// zkr_book.hip -- the book of a ledger: the state RollUp.sol keeps by public key beside its tree, on the GPU.
// deposit(publicKeyX, publicKeyY) (contracts/contracts/RollUp.sol:255-297 of the reference), withdraw / withdrawAll (:193-253) and
// accuredFees (:139, :299-309) for whole lists of calls:
//
//   a  key hashes     one thread per key: hashPair(pubX, pubY) (mimc_device.hpp mimc_hash_pair), of the ledger's records (the key
//                     table) or of a call list
//   b  claim          "insert n keys into a slot table, the lowest position wins": the key table, the nullifier table, and a
//                     scratch table per call list that gives every entry its leader -- the lowest list position with its key
//   c  resolve        one thread per call entry, in a LATER launch: words below r, the key's account, nullifier spent, leader
//   d  host pass      book_plan.cpp: the contract's checks and balance arithmetic in list order
//   e  apply          the applied calls' events are an update list for the storing path of zkr_ledger_deposit
//                     (ledger_apply_updates in zkr_sequencer.hip: tables, then stage_updates and store_updates)
//
// Every probe loop below is a `for` over at most the table's capacity, and the host establishes a load factor of at most 1/2
// before a launch that inserts.  The claim writes slot words only (the keys are in place before the launch), with ordinary
// device-scope atomics on uint32_t; nothing reads a slot it did not just exchange until the next launch.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "zkr_internal.hpp"
#include "rollup_witness.hpp"
#include "mimc_device.hpp"
#include "ledger_internal.hpp"
#include "book_plan.hpp"

namespace zkr {

// ------------------------------------------------------------------------------------------------ a. key hashes
// out[i] = multiHash(keys[i * stride], keys[i * stride + 1]), standard form in and out.  A key with an element not below r is no
// key of the contract's field: it gets all ones, which no hash is (not below r), so that it can never share a table entry or a
// leader with the key it is congruent to.
static __global__ __launch_bounds__(64) void book_keyhash_kernel(const Fr *keys, size_t stride, size_t n, Fr *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr x = keys[i * stride], y = keys[i * stride + 1];
  Fr h;
  if (!words_below(x.v, FrParams::P) || !words_below(y.v, FrParams::P)) {
#pragma unroll
    for (int j = 0; j < 8; j++) h.v[j] = 0xFFFFFFFFu;
  } else h = mimc_hash_pair(x, y);
  out[i] = h;
}

// ------------------------------------------------------------------------------------------------ b, c. tables
// Where a key's probe starts.  A key hash is a MiMC output, uniform already: its low word.  A nullifier is chosen by its user:
// all eight words, mixed with the book's salt.
__device__ __forceinline__ uint32_t book_slot(const Fr &k, uint64_t salt, uint32_t mixed) {
  if (!mixed) return k.v[0];
  uint64_t h = salt;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    h = (h ^ k.v[i]) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
  }
  h = (h ^ (h >> 29)) * 0xBF58476D1CE4E5B9ull;
  return (uint32_t)(h ^ (h >> 32));
}
// Thread t inserts key i = first + t of `keys` (stride in elements) into tab (mask + 1 slots, a power of two; a slot holds
// position + 1, 0 = empty).  An empty slot is taken by compare-and-swap; at an occupied one the owner's key is compared: equal ->
// the slot keeps the lower position and the thread is done, different -> the next slot, wrapping.  A slot never empties and the
// key it stands for never changes, so all holders of one key stop at the same slot whatever the schedule, and it ends holding the
// lowest of them.  *taken counts the slots this launch took (distinct new keys).  At most mask + 1 steps.
static __global__ __launch_bounds__(256) void book_claim_kernel(uint32_t *tab, uint32_t mask, const Fr *keys, size_t stride, size_t first, size_t n, uint64_t salt,
                                                                uint32_t mixed, uint32_t *taken) {
  const size_t i = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fr key = keys[i * stride];
  uint32_t s = book_slot(key, salt, mixed) & mask;
  for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
    const uint32_t cur = atomicCAS(&tab[s], 0u, (uint32_t)i + 1);
    if (cur == 0) {
      if (taken) atomicAdd(taken, 1u);
      return;
    }
    if ((size_t)cur - 1 >= n) return;  // no slot holds that: nothing to follow
    if (keys[((size_t)cur - 1) * stride] == key) {
      atomicMin(&tab[s], (uint32_t)i + 1);
      return;
    }
  }
}
// The slot word of `key` in a table that an earlier launch completed, or 0.  At most mask + 1 steps.
__device__ __forceinline__ uint32_t book_find(const uint32_t *tab, uint32_t mask, const Fr *keys, size_t stride, size_t n_keys, const Fr &key, uint64_t salt, uint32_t mixed) {
  uint32_t s = book_slot(key, salt, mixed) & mask;
  for (uint32_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
    const uint32_t cur = tab[s];
    if (cur == 0 || (size_t)cur - 1 >= n_keys) return 0;
    if (keys[((size_t)cur - 1) * stride] == key) return cur;
  }
  return 0;
}
struct BookTable {  // a slot table and the keys its slots name; tab == nullptr: this part of the question is not asked
  const uint32_t *tab;
  uint32_t mask, mixed;
  const Fr *keys;
  size_t stride, n_keys;
};
struct BookQuery {
  const Fr *pubs;      // entry i's key at pubs[i * pub_stride], + 1; or null
  size_t pub_stride;
  const Fr *keyhash;   // n: the hash of entry i's key (book_keyhash_kernel), where pubs is set
  const Fr *nulls;     // entry i's nullifier at nulls[i * null_stride]; or null
  size_t null_stride;
  BookTable accounts;  // the persistent key table over d_keyhash
  BookTable spent;     // the persistent nullifier table over d_null
  BookTable scratch;   // the call list's own table: over keyhash (deposits) or over the nullifiers (withdrawals)
  uint64_t salt;
  size_t n;
};
static __global__ __launch_bounds__(256) void book_resolve_kernel(BookQuery q, BookResolve *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n) return;
  BookResolve r{0, BOOK_NONE, (uint32_t)i};
  if (q.pubs) {
    const Fr x = q.pubs[i * q.pub_stride], y = q.pubs[i * q.pub_stride + 1];
    if (words_below(x.v, FrParams::P)) r.flags |= BOOK_X_BELOW_R;
    if (words_below(y.v, FrParams::P)) r.flags |= BOOK_Y_BELOW_R;
    if (q.accounts.tab) {
      const uint32_t at = book_find(q.accounts.tab, q.accounts.mask, q.accounts.keys, 1, q.accounts.n_keys, q.keyhash[i], 0, 0);
      if (at) r.account = at - 1;
    }
  }
  if (q.nulls) {
    const Fr nul = q.nulls[i * q.null_stride];
    if (words_below(nul.v, FrParams::P)) r.flags |= BOOK_NULL_BELOW_R;
    if (q.spent.tab && book_find(q.spent.tab, q.spent.mask, q.spent.keys, 1, q.spent.n_keys, nul, q.salt, 1)) r.flags |= BOOK_NULL_USED;
  }
  if (q.scratch.tab) {
    const Fr key = q.scratch.keys[i * q.scratch.stride];
    const uint32_t at = book_find(q.scratch.tab, q.scratch.mask, q.scratch.keys, q.scratch.stride, q.scratch.n_keys, key, q.salt, q.scratch.mixed);
    if (at) r.leader = at - 1;
  }
  out[i] = r;
}
// Words 1..3 of witness i -> entry i's public signals [publicKey[0], publicKey[1], nullifier] (withdraw.circom), one thread per
// word: where zkr_verify_each_device reads them, as replay_gather_kernel does for a batch.
static __global__ __launch_bounds__(256) void book_signals_kernel(const Fr *const *witnesses, size_t n, Fr *out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 3 * n) return;
  out[g] = witnesses[g / 3][1 + g % 3];
}

// ------------------------------------------------------------------------------------------------ host side
namespace {
enum : size_t { BOOK_PIECE = (size_t)1 << 20, BOOK_MAX_CALLS = (size_t)1 << 22 };

uint32_t pow2_at_least(size_t v) {
  uint32_t c = 4;
  while (c < v) c <<= 1;
  return c;
}
int launch_claim(uint32_t *tab, uint32_t cap, const Fr *keys, size_t stride, size_t first, size_t n, uint64_t salt, uint32_t mixed, uint32_t *taken, hipStream_t s) {
  if (n <= first) return ZKR_OK;
  if (2 * n > cap) { set_error("internal: %zu keys for a table of %u slots", n, cap); return ZKR_ERR_ARG; }  // the bound that ends every probe
  book_claim_kernel<<<blocks(n - first, 256), 256, 0, s>>>(tab, cap - 1, keys, stride, first, n, salt, mixed, taken);
  ZKR_HIP_CHECK(hipGetLastError());
  return ZKR_OK;
}

// d_keyhash[first .. last) from the ledger's records, then their slots.  The arena is used for staging.
int keys_extend(zkr_ledger *l, size_t first, size_t last) {
  LedgerBook *b = l->book;
  if (last <= first) return ZKR_OK;
  const size_t piece = last - first < BOOK_PIECE ? last - first : (size_t)BOOK_PIECE;
  int rc = l->arena.reserve(DevArena::padded(piece * 128) + DevArena::padded(4));
  if (rc) return rc;
  Fr *d_stage = l->arena.take<Fr>(piece * 4);
  uint32_t *d_taken = l->arena.take<uint32_t>(1), taken = 0;
  for (size_t at = first; at < last; at += piece) {
    const size_t n = last - at < piece ? last - at : piece;
    ZKR_HIP_CHECK(hipMemcpy(d_stage, l->records.data() + at * 128, n * 128, hipMemcpyHostToDevice));
    book_keyhash_kernel<<<blocks(n, 64), 64>>>(d_stage, 4, n, b->d_keyhash + at);
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipDeviceSynchronize());  // the staging is written again
  }
  ZKR_HIP_CHECK(hipMemset(d_taken, 0, 4));
  if ((rc = launch_claim(b->d_keytab, (uint32_t)2 << l->depth, b->d_keyhash, 1, first, last, 0, 0, d_taken, nullptr))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(&taken, d_taken, 4, hipMemcpyDeviceToHost));
  b->distinct += taken;
  return ZKR_OK;
}
int nulls_rebuild(LedgerBook *b) {
  ZKR_HIP_CHECK(hipMemset(b->d_nulltab, 0, b->null_cap * 4));
  int rc = launch_claim(b->d_nulltab, (uint32_t)b->null_cap, b->d_null, 1, 0, b->null_count, b->salt, 1, nullptr, nullptr);
  if (rc) return rc;
  ZKR_HIP_CHECK(hipDeviceSynchronize());
  b->null_stale = false;
  return ZKR_OK;
}
// Both tables say what the records and the nullifier array say: the step in front of every by-key call.
int book_fresh(zkr_ledger *l) {
  LedgerBook *b = l->book;
  if (b->keys_stale) {
    ZKR_HIP_CHECK(hipMemset(b->d_keytab, 0, ((size_t)2 << l->depth) * 4));
    b->distinct = 0;
    int rc = keys_extend(l, 0, l->accounts);
    if (rc) return rc;
    ZKR_HIP_CHECK(hipDeviceSynchronize());
    b->keys_stale = false, b->rebuilds++;
  }
  if (b->null_stale) return nulls_rebuild(b);
  return ZKR_OK;
}
// count + inserts <= capacity / 2 before a launch that inserts: otherwise the table doubles and the array is inserted again.
// Nothing of the book moves until the new table is complete.
int nulls_room(LedgerBook *b, size_t inserts) {
  size_t cap = b->null_cap;
  while (b->null_count + inserts > cap / 2) cap *= 2;
  if (cap == b->null_cap) return ZKR_OK;
  if (cap > ((size_t)1 << 31)) { set_error("the nullifier set cannot hold %zu entries", b->null_count + inserts); return ZKR_ERR_ARG; }
  Dev<Fr> arr;
  Dev<uint32_t> tab;
  if (arr.alloc(cap / 2) || tab.alloc(cap)) {
    set_error("out of device memory for a nullifier table of %zu slots", cap);
    return ZKR_ERR_HIP;
  }
  hipError_t e = b->null_count ? hipMemcpy(arr, b->d_null, b->null_count * 32, hipMemcpyDeviceToDevice) : hipSuccess;
  if (e == hipSuccess) e = hipMemset(tab, 0, cap * 4);
  int rc = ZKR_OK;
  if (e == hipSuccess) rc = launch_claim(tab, (uint32_t)cap, arr, 1, 0, b->null_count, b->salt, 1, nullptr, nullptr);
  if (e == hipSuccess && !rc) e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("growing the nullifier table failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  if (rc) return rc;
  b->d_null = std::move(arr), b->d_nulltab = std::move(tab), b->null_cap = cap, b->null_room = cap / 2, b->null_stale = false;
  return ZKR_OK;
}

struct Ask {
  const uint8_t *host = nullptr;         // n x stride x 32 B in host memory, or
  const void *const *witnesses = nullptr;  // n device pointers (stride 3)
  size_t stride = 0, n = 0;
  bool pubs = false, nulls = false, leaders = false;
};
// Steps a-c for one list.  res: n entries; gathered (device form): the signals as the host pass reads them.
int resolve(zkr_ledger *l, const Ask &a, hipStream_t s, std::vector<BookResolve> &res, std::vector<uint8_t> *gathered) {
  LedgerBook *b = l->book;
  int rc = book_fresh(l);
  if (rc) return rc;
  const size_t n = a.n;
  const uint32_t cap = a.leaders ? pow2_at_least(2 * n) : 0;
  rc = l->arena.reserve(DevArena::padded(n * a.stride * 32) + DevArena::padded(n * 32) + DevArena::padded((size_t)cap * 4) + DevArena::padded(n * sizeof(BookResolve)) +
                        DevArena::padded(n * sizeof(void *)));
  if (rc) return rc;
  Fr *d_in = l->arena.take<Fr>(n * a.stride), *d_hash = l->arena.take<Fr>(n);
  uint32_t *d_scratch = l->arena.take<uint32_t>(cap);
  BookResolve *d_res = l->arena.take<BookResolve>(n);
  const Fr **d_ptrs = l->arena.take<const Fr *>(n);
  if (a.host) ZKR_HIP_CHECK(hipMemcpyAsync(d_in, a.host, n * a.stride * 32, hipMemcpyHostToDevice, s));
  else {
    ZKR_HIP_CHECK(hipMemcpyAsync(d_ptrs, a.witnesses, n * sizeof(void *), hipMemcpyHostToDevice, s));
    book_signals_kernel<<<blocks(3 * n, 256), 256, 0, s>>>(d_ptrs, n, d_in);
    ZKR_HIP_CHECK(hipGetLastError());
    gathered->resize(n * 96);
    ZKR_HIP_CHECK(hipMemcpyAsync(gathered->data(), d_in, n * 96, hipMemcpyDeviceToHost, s));
  }
  BookQuery q;
  memset(&q, 0, sizeof q);
  q.n = n, q.salt = b->salt;
  if (a.pubs) {
    book_keyhash_kernel<<<blocks(n, 64), 64, 0, s>>>(d_in, a.stride, n, d_hash);
    ZKR_HIP_CHECK(hipGetLastError());
    q.pubs = d_in, q.pub_stride = a.stride, q.keyhash = d_hash;
    q.accounts = BookTable{b->d_keytab, ((uint32_t)2 << l->depth) - 1, 0, b->d_keyhash, 1, l->accounts};
  }
  if (a.nulls) {
    q.nulls = d_in + (a.pubs ? 2 : 0), q.null_stride = a.stride;
    q.spent = BookTable{b->d_nulltab, (uint32_t)b->null_cap - 1, 1, b->d_null, 1, b->null_count};
  }
  if (a.leaders) {
    const Fr *keys = a.nulls ? q.nulls : d_hash;
    const size_t stride = a.nulls ? a.stride : 1;
    ZKR_HIP_CHECK(hipMemsetAsync(d_scratch, 0, (size_t)cap * 4, s));
    if ((rc = launch_claim(d_scratch, cap, keys, stride, 0, n, b->salt, a.nulls ? 1 : 0, nullptr, s))) return rc;
    q.scratch = BookTable{d_scratch, cap - 1, a.nulls ? 1u : 0u, keys, stride, n};
  }
  book_resolve_kernel<<<blocks(n, 256), 256, 0, s>>>(q, d_res);  // a later launch than every claim it reads
  ZKR_HIP_CHECK(hipGetLastError());
  res.resize(n);
  ZKR_HIP_CHECK(hipMemcpyAsync(res.data(), d_res, n * sizeof(BookResolve), hipMemcpyDeviceToHost, s));
  ZKR_HIP_CHECK(hipStreamSynchronize(s));
  return ZKR_OK;
}

int open_checks(const zkr_ledger *l, size_t n, const char *what) {
  if (!l->book) { set_error("%s: the ledger has no open book (zkr_ledger_book_open)", what); return ZKR_ERR_ARG; }
  if (n > BOOK_MAX_CALLS) { set_error("%s: more than 2^22 entries in one call", what); return ZKR_ERR_ARG; }
  return ZKR_OK;
}
void plan_out(const BookPlan &plan, size_t n, uint8_t *status, uint32_t *indices, uint8_t *events) {
  memcpy(status, plan.status.data(), n);
  if (indices) memcpy(indices, plan.index.data(), n * sizeof(uint32_t));
  if (events) memcpy(events, plan.events.data(), n * 128);
}

int withdraw_calls(zkr_ledger *l, const uint8_t *publics, const void *const *d_witnesses, const uint8_t *amounts, const uint8_t *proof_verdicts, size_t n,
                   uint8_t *verdicts, uint32_t *indices, uint8_t *events, hipStream_t s) {
  if (!l || (n && ((!publics && !d_witnesses) || !verdicts))) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  int rc = open_checks(l, n, "withdraw calls");
  if (rc) return rc;
  for (size_t i = 0; d_witnesses && i < n; i++)
    if (!d_witnesses[i]) { set_error("witness %zu is a null pointer", i); return ZKR_ERR_ARG; }
  if (n == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  LedgerBook *b = l->book;
  Ask a;
  a.host = publics, a.witnesses = d_witnesses, a.stride = 3, a.n = n, a.pubs = a.nulls = a.leaders = true;
  std::vector<BookResolve> res;
  std::vector<uint8_t> gathered;
  if ((rc = resolve(l, a, s, res, &gathered))) return rc;
  if (!publics) publics = gathered.data();
  BookPlan plan;
  const char *why = "";
  if (withdraw_plan(l->records.data(), l->accounts, publics, amounts, proof_verdicts, n, res.data(), plan, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  const size_t m = plan.accepted.size();
  if (m) {
    if ((rc = nulls_room(b, m))) return rc;
    std::vector<uint8_t> fresh(m * 32);  // behind the array's end: not part of the set until the count moves
    for (size_t k = 0; k < m; k++) memcpy(&fresh[k * 32], publics + (size_t)plan.accepted[k] * 96 + 64, 32);
    ZKR_HIP_CHECK(hipMemcpy(b->d_null + b->null_count, fresh.data(), m * 32, hipMemcpyHostToDevice));
    if ((rc = ledger_apply_updates(l, plan.upd_idx.data(), plan.upd_rec.data(), m, l->accounts))) return rc;
    b->null_count += m;  // the ledger has moved: from here on a failure can only leave a table to be rebuilt
    if (launch_claim(b->d_nulltab, (uint32_t)b->null_cap, b->d_null, 1, b->null_count - m, b->null_count, b->salt, 1, nullptr, nullptr) || hipDeviceSynchronize() != hipSuccess)
      b->null_stale = true;
  }
  plan_out(plan, n, verdicts, indices, events);
  return ZKR_OK;
}
}  // namespace

}  // namespace zkr

using namespace zkr;

extern "C" {

int zkr_ledger_book_open(zkr_ledger *l, const zkr_book_opts *opts, const void *blob, size_t blob_len) {
  if (!l || (!blob && blob_len)) { set_error("null argument"); return ZKR_ERR_ARG; }
  const uint32_t cap_log2 = opts && opts->nullifier_cap_log2 ? opts->nullifier_cap_log2 : 10;
  if (cap_log2 < 2 || cap_log2 > 31 || (opts && opts->reserved)) { set_error("book options: nullifier_cap_log2 %u out of range (2..31), or a reserved word that is not zero", cap_log2); return ZKR_ERR_ARG; }
  BookHeader h;
  char why[200];
  if (blob && book_blob_parse((const uint8_t *)blob, blob_len, &h, why, sizeof why)) { set_error("%s", why); return ZKR_ERR_ARG; }  // before the device is looked at
  if (h.count > ((uint64_t)1 << 30)) { set_error("book blob: %llu nullifiers are more than a table of 2^31 slots holds", (unsigned long long)h.count); return ZKR_ERR_ARG; }
  uint64_t salt = opts ? opts->salt : 0;
  int rc = salt ? ZKR_OK : os_random(&salt, 8);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(l->mu);
  if (l->book) { set_error("the ledger's book is open already"); return ZKR_ERR_ARG; }
  if ((rc = need_device(l->device, "the ledger's book"))) return rc;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  if ((rc = upload_mimc_constants(l->device))) return rc;
  LedgerBook *b = new LedgerBook;
  b->salt = salt, b->null_cap = (size_t)1 << cap_log2, b->null_count = (size_t)h.count;
  while (b->null_count > b->null_cap / 2) b->null_cap *= 2;
  b->null_room = b->null_cap / 2;
  memcpy(b->fees.w, h.fees, 32);
  l->book = b;
  auto fail = [&](int code) {
    delete b;
    l->book = nullptr;
    return code;
  };
  if (b->d_keyhash.alloc((size_t)1 << l->depth) || b->d_keytab.alloc((size_t)2 << l->depth) || b->d_null.alloc(b->null_room) || b->d_nulltab.alloc(b->null_cap)) {
    set_error("out of device memory for the book of a ledger of depth %u", l->depth);
    return fail(ZKR_ERR_HIP);
  }
  if (b->null_count && hipMemcpy(b->d_null, (const uint8_t *)blob + BOOK_HEADER_BYTES, b->null_count * 32, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("the blob's nullifiers did not reach the device");
    return fail(ZKR_ERR_HIP);
  }
  b->keys_stale = b->null_stale = true;
  if ((rc = book_fresh(l))) return fail(rc);
  if (b->null_count) {  // one nullifier twice: an entry whose leader in the set's own table is another one
    std::vector<BookResolve> res;
    const size_t n = b->null_count;
    if ((rc = l->arena.reserve(DevArena::padded(n * sizeof(BookResolve))))) return fail(rc);
    BookResolve *d_res = l->arena.take<BookResolve>(n);
    BookQuery q;
    memset(&q, 0, sizeof q);
    q.n = n, q.salt = b->salt;
    q.scratch = BookTable{b->d_nulltab, (uint32_t)b->null_cap - 1, 1, b->d_null, 1, n};
    book_resolve_kernel<<<blocks(n, 256), 256>>>(q, d_res);
    res.resize(n);
    if (hipGetLastError() != hipSuccess || hipMemcpy(res.data(), d_res, n * sizeof(BookResolve), hipMemcpyDeviceToHost) != hipSuccess) {
      set_error("looking for repeated nullifiers failed");
      return fail(ZKR_ERR_HIP);
    }
    for (size_t i = 0; i < n; i++)
      if (res[i].leader != i) {
        set_error("book blob: nullifier %zu repeats nullifier %u", i, res[i].leader);
        return fail(ZKR_ERR_BAD_KEY);
      }
  }
  return ZKR_OK;
}

int zkr_ledger_book_info(const zkr_ledger *l, uint64_t out[4]) {
  if (!l || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  int rc = open_checks(l, 0, "book info");
  if (rc) return rc;
  zkr_ledger *m = const_cast<zkr_ledger *>(l);  // a stale table is rebuilt: what is reported is what the records say
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  if ((rc = book_fresh(m))) return rc;
  out[0] = l->book->distinct, out[1] = l->book->null_count, out[2] = l->book->null_cap, out[3] = l->book->rebuilds;
  return ZKR_OK;
}

int zkr_ledger_deposit_calls(zkr_ledger *l, const uint8_t *pubs, const uint8_t *values, size_t n, uint8_t *status, uint32_t *indices, uint8_t *events) {
  if (!l || (n && (!pubs || !values || !status))) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  int rc = open_checks(l, n, "deposit calls");
  if (rc) return rc;
  if (n == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  Ask a;
  a.host = pubs, a.stride = 2, a.n = n, a.pubs = a.leaders = true;
  std::vector<BookResolve> res;
  if ((rc = resolve(l, a, nullptr, res, nullptr))) return rc;
  BookPlan plan;
  const char *why = "";
  if (deposit_plan(l->depth, l->records.data(), l->accounts, pubs, values, n, res.data(), plan, &why)) { set_error("%s", why); return ZKR_ERR_ARG; }
  const size_t before = l->accounts, m = plan.upd_idx.size();
  if (m) {
    if ((rc = ledger_apply_updates(l, plan.upd_idx.data(), plan.upd_rec.data(), m, plan.accounts_after))) return rc;
    // the new accounts' hashes and slots; the ledger has moved, so a failure here only leaves the table to be rebuilt
    if (keys_extend(l, before, l->accounts) || hipDeviceSynchronize() != hipSuccess) l->book->keys_stale = true;
  }
  plan_out(plan, n, status, indices, events);
  return ZKR_OK;
}

int zkr_ledger_withdraw_calls(zkr_ledger *l, const uint8_t *publics, const uint8_t *amounts, const uint8_t *proof_verdicts, size_t n, uint8_t *verdicts,
                              uint32_t *indices, uint8_t *events) {
  if (n && !publics) { set_error("null argument"); return ZKR_ERR_ARG; }
  return withdraw_calls(l, publics, nullptr, amounts, proof_verdicts, n, verdicts, indices, events, nullptr);
}

int zkr_ledger_withdraw_calls_device(zkr_ledger *l, const void *const *d_witnesses_std, const uint8_t *amounts, const uint8_t *proof_verdicts, size_t n,
                                     uint8_t *verdicts, uint32_t *indices, uint8_t *events, void *stream) {
  if (n && !d_witnesses_std) { set_error("null argument"); return ZKR_ERR_ARG; }
  return withdraw_calls(l, nullptr, d_witnesses_std, amounts, proof_verdicts, n, verdicts, indices, events, (hipStream_t)stream);
}

int zkr_ledger_lookup_keys(zkr_ledger *l, const uint8_t *pubs, size_t n, uint32_t *indices) {
  if (!l || (n && (!pubs || !indices))) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  int rc = open_checks(l, n, "key look-up");
  if (rc) return rc;
  if (n == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  Ask a;
  a.host = pubs, a.stride = 2, a.n = n, a.pubs = true;
  std::vector<BookResolve> res;
  if ((rc = resolve(l, a, nullptr, res, nullptr))) return rc;
  for (size_t i = 0; i < n; i++) {
    const bool held = res[i].account < l->accounts && !memcmp(l->records.data() + (size_t)res[i].account * 128, pubs + i * 64, 64);
    indices[i] = held ? res[i].account : BOOK_NONE;
  }
  return ZKR_OK;
}

int zkr_ledger_nullifiers_used(zkr_ledger *l, const uint8_t *nullifiers, size_t n, uint8_t *used) {
  if (!l || (n && (!nullifiers || !used))) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  int rc = open_checks(l, n, "nullifier look-up");
  if (rc) return rc;
  if (n == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(l->device));
  Ask a;
  a.host = nullifiers, a.stride = 1, a.n = n, a.nulls = true;
  std::vector<BookResolve> res;
  if ((rc = resolve(l, a, nullptr, res, nullptr))) return rc;
  for (size_t i = 0; i < n; i++) used[i] = (res[i].flags & BOOK_NULL_USED) ? 1 : 0;
  return ZKR_OK;
}

int zkr_ledger_fees(const zkr_ledger *l, uint8_t fees[32], int reset) {
  if (!l || !fees) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  int rc = open_checks(l, 0, "fees");
  if (rc) return rc;
  if (reset && l->journal.open()) { set_error("the fee counter cannot be reset while a checkpoint is open: a rollback could not put it back"); return ZKR_ERR_ARG; }
  memcpy(fees, l->book->fees.w, 32);
  if (reset) l->book->fees = int256_small(0);
  return ZKR_OK;
}

int zkr_ledger_book_blob(const zkr_ledger *l, void **blob, size_t *len) {
  if (blob) *blob = nullptr;
  if (!l || !blob || !len) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(l->mu);
  int rc = open_checks(l, 0, "book blob");
  if (rc) return rc;
  const LedgerBook *b = l->book;
  BookHeader h;
  h.count = b->null_count;
  memcpy(h.fees, b->fees.w, 32);
  const size_t n = BOOK_HEADER_BYTES + b->null_count * 32;
  uint8_t *out = (uint8_t *)malloc(n);
  if (!out) { set_error("out of memory for a book blob of %zu bytes", n); return ZKR_ERR_ARG; }
  if (book_header_write(h, out)) { free(out); set_error("the blob's tag could not be computed"); return ZKR_ERR_ARG; }
  if (b->null_count) {
    hipError_t e = hipSetDevice(l->device);
    if (e == hipSuccess) e = hipMemcpy(out + BOOK_HEADER_BYTES, b->d_null, b->null_count * 32, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(out); set_error("reading the nullifiers failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  }
  *blob = out, *len = n;
  return ZKR_OK;
}

}  // extern "C"
