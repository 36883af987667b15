// zkr_internal.hpp -- host-side structures shared by the translation units of libzkr_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>
#include "../../include/zkr.h"
#include "hostops.hpp"
#include "zkr_owners.hpp"
#include "msm_plan.hpp"
#include "qap_forms.hpp"
#include "shard_group.hpp"

namespace zkr {

struct Tw29;  // kernels_ntt.hpp: a butterfly twiddle as nine 29-bit limbs
int os_random(void *out, size_t bytes);  // `bytes` from the OS CSPRNG (zkr_key.hip, beside set_error); ZKR_ERR_ARG with a message when it cannot be read
// ZKR_H_FORM=coefficients: no side tables are built and every proof takes the coefficient form.  Read at every call, kept nowhere
inline bool h_form_forced_coefficients() { const char *e = getenv("ZKR_H_FORM"); return e && !strcmp(e, "coefficients"); }
// every entry point that needs a GPU refuses the same way when there is none
inline int need_device(int device) {
  const int found = zkr_device_count();
  if (found <= device || device < 0) { set_error("no HIP device %d (found %d); libzkr_hip has no CPU fallback", device, found); return ZKR_ERR_NO_DEVICE; }
  return 0;
}
// the same for a call that has a name of its own: `what`, with the host call that does the same job where there is one
inline unsigned blocks_of(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }  // of a one-thread-per-item launch
inline int need_device(int device, const char *what) {
  if (zkr_device_count() <= device || device < 0) { set_error("no HIP device %d; %s runs on the GPU and has no CPU fallback", device, what); return ZKR_ERR_NO_DEVICE; }
  return 0;
}

// "How many are bad, and which comes first": the two words a checking kernel updates with group_note_bad (kernels_group.hpp).
struct FaultCounter {
  DevBuf buf;
  uint32_t count = 0, first = 0xffffffffu;  // as of the last read()
  uint32_t *dev() const { return buf.as<uint32_t>(); }
  int reset() {  // before every launch
    if (!buf.p)
      if (int rc = buf.alloc(8)) return rc;
    const uint32_t none[2] = {0u, 0xffffffffu};
    ZKR_HIP_CHECK(hipMemcpy(buf.p, none, 8, hipMemcpyHostToDevice));
    return 0;
  }
  int read() {  // after the launch: its launch error, if any, or its tally
    uint32_t res[2];
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpy(res, buf.p, 8, hipMemcpyDeviceToHost));
    count = res[0]; first = res[1];
    return 0;
  }
};

// The device key is ONE position-independent arena: header + sections addressed by byte offsets,
// so a replica on another GPU is a single broadcast of [arena, arena+len).
struct ArenaHeader {
  uint64_t magic;      // "ZKRKEY04"
  uint64_t total_len;
  uint32_t n, p, m, logm;
  uint32_t nnzA, nnzB;
  uint32_t npts[N_TABLES];
  uint32_t tlog;       // twiddle table entries = 2^tlog (= m)
  uint64_t off_tw, off_twl;
  uint64_t off_rowptr[2], off_col[2], off_coef[2];
  uint64_t off_wide[2];  // row indices of the QAP rows wider than SPMV_WIDE terms (spmv_wide_kernel)
  uint32_t n_wide[2];
  uint64_t off_pts[N_TABLES], off_rank[N_TABLES];  // rank: u32 per scalar of the table's vector -> index of its point, RANK_NONE if dropped
  uint8_t alfa1[64], beta1[64], delta1[64];  // Montgomery affine, as in the websnark key header
  uint8_t beta2[128], delta2[128];
  uint32_t share_b;    // B1 and B2 keep the same signals (always true for honest keys): one digit sort serves both
  uint32_t win_c[N_TABLES];  // window bits of each table: off_pts[t] holds K = ceil(255/c) x npts[t] points, level k = 2^(ck) * base
  uint32_t share_ac;   // A and C are laid out over the union of their supports (missing points stored as infinity): one digit sort serves both
  uint32_t rank_identity[N_TABLES];  // rank[s] == s for every scalar of the table's vector: the sort skips the gather
  // Intra-proof sharding (zkr_key_shard): a shard key multiplies only the scalars [sc_lo, sc_lo + sc_n) of
  // each scalar vector (index 0: the witness w, serving A, B1, B2, C; index 1: h, serving H) and holds only their points; its rank
  // maps have sc_n entries (rank[i] = point of scalar sc_lo + i).  A whole key: sc_lo = 0, sc_n = {n, m}, shard_parts = 1.
  uint32_t sc_lo[2], sc_n[2];
  uint32_t shard_part, shard_parts;
};
static_assert(sizeof(ArenaHeader) <= 1024, "header fits its slot");
constexpr size_t ARENA_HEADER_BYTES = 1024;
constexpr uint64_t ARENA_MAGIC = 0x343059454b524b5aull;  // "ZKRKEY04" (03: point tables in the radix-2^261 form of field29.hpp; 04: scalar sub-ranges of shard keys): bump with every change of ArenaHeader or of a section layout (packed key files carry it)
inline uint32_t rank_entries(const ArenaHeader &h, int t) { return h.sc_n[t == T_H ? 1 : 0]; }  // entries of table t's rank map = scalars the key multiplies with it
// the 448 bytes of constants in a websnark key's header <-> the header's fields
inline void header_set_consts(ArenaHeader &h, const uint8_t *consts448) {
  memcpy(h.alfa1, consts448, 64); memcpy(h.beta1, consts448 + 64, 64); memcpy(h.delta1, consts448 + 128, 64);
  memcpy(h.beta2, consts448 + 192, 128); memcpy(h.delta2, consts448 + 320, 128);
}
inline void header_get_consts(const ArenaHeader &h, uint8_t *consts448) {
  memcpy(consts448, h.alfa1, 64); memcpy(consts448 + 64, h.beta1, 64); memcpy(consts448 + 128, h.delta1, 64);
  memcpy(consts448 + 192, h.beta2, 128); memcpy(consts448 + 320, h.delta2, 128);
}
// bytes the caller frees with zkr_free: a malloc'ed copy of v.  ZKR_ERR_ARG with the out-pointers null when there is no memory
inline int give_bytes(const std::vector<uint8_t> &v, void **out, size_t *len) {
  *out = malloc(v.size() ? v.size() : 1);
  *len = 0;
  if (!*out) { set_error("out of memory"); return ZKR_ERR_ARG; }
  if (!v.empty()) memcpy(*out, v.data(), v.size());
  *len = v.size();
  return 0;
}

// digit records of one scalar vector, split by bucket range (kernels_msm.hpp "digit sort", stage 1)
struct DigitLists {
  Dev<uint32_t> rng;  // counts[range][XCD slot] | fill cursors[range][XCD slot] | range offsets[nR + 1]  (kernels_msm.hpp DIGIT_RNG_WORDS)
  Dev<uint32_t> ent_s, ent_b;
};

// The digit sort of one point set: bucket occupancies, offsets and the sorted entry list, read by the accumulation of every table over
// that point set (B2 over B1's, C over A's: ProofLayout::sort_src) and by their oversized-bucket kernels.
struct MsmSort {
  Dev<uint32_t> counts, offsets, entries;
  Dev<uint32_t> size_hist, order;  // [2][SIZE_BINS] size-class histogram + hand-out counters; bucket ids fullest first
  Dev<uint32_t> chunk_cnt;  // [K][J][nbw] per-chunk bucket occupancies, then per-bucket prefixes over chunks
  Dev<uint32_t> big_list, big_count, block_sums;
  size_t max_nb = 0, max_entries = 0;
};
// One reduction chain: `sets` bucket sets per proof end to end (the fused proofs of each set together) with the buffers of the
// launch set that reduces them (ChainLayout).  result / h_result: one point per set and proof, set-major.
struct MsmChain {
  DevBuf buckets, group_out, task_out, result;
  PinnedBuf h_result;  // pinned host copy of the result points (XYZZ)
  size_t sets = 1;
  bool g2 = false;
};
// One table multiplied on its own (the stage hooks zkr_msm_g1 / g2, key_table_msm): its digit records, sort, oversized-bucket
// partial sums and chain, all of which go with the scope -- the hooks return early on every failed HIP call
struct MsmScratch {
  DigitLists dig;
  MsmSort sort;
  DevBuf big_partials;
  MsmChain chain;
};

struct ProfStage {
  std::string name;
  double ms = 0;
  uint64_t launches = 0;
};
struct ProfSpan {
  int stage;
  hipEvent_t e0, e1;
};

}  // namespace zkr

namespace zkr {
// Everything one proof in flight owns: witness + calcH vectors, digit codes, the sorts, partial sums and chains of its MSMs, its
// events and timing spans.  A key has PROOF_SLOTS of them so that the GPU work of the next proof is enqueued
// (zkr_prove_submit) while the host still assembles the previous one (zkr_prove_collect).
constexpr int PROOF_SLOTS = 2;  // three measured the same (134.1 against 134.1 / 134.3 proofs/s, HISTORY.md 7b)
constexpr int MAX_FUSE = 16;  // most proofs one launch set carries (zkr_key.hip fused_capacity)
// Host witnesses (zkr_prove, zkr_prove_batch: the ArrayBuffer of binarifyWitness) reach the GPU through a ring of device
// staging buffers, one more than there are proof slots: the witness of the NEXT proof crosses PCIe while both slots
// compute (and outside the key's lock), so a stream of host-buffer calls keeps the GPU as busy as device-resident
// witnesses do.
constexpr int STAGE_BUFS = PROOF_SLOTS + 1;
struct WitnessStage {
  Dev<Fr> d_w;         // its device copy, read by ingest_kernel
  ScopedEvent ev_up;
  bool busy = false;
};
struct ProofSlot {
  Dev<Fr> d_w, va, vb, ca, cb, d_h;
  DigitLists dig_w, dig_h;  // digit records of w (shared by A, B1, B2, C) and of h
  MsmSort sort[N_TABLES];          // of the tables that own their sort (layout.sort_src[t] == t) and have points
  DevBuf big_partials[N_TABLES];  // oversized-bucket partial sums of every table that has points
  MsmChain chain[N_TABLES];        // the first layout.n_chains of them
  ScopedEvent ev_w, ev_h;
  ScopedEvent ev_end[3];  // end of the proof's work on the G2-chain, G1-chain and auxiliary streams
  ScopedEvent ev_done[N_TABLES], ev_sorted[N_TABLES];
  ScopedEvent ev_res[N_TABLES];  // by chain: its result points have landed in its pinned host buffer
  bool res_pending[N_TABLES] = {false, false, false, false, false};
  int cap = 1;    // proofs one submit can fuse into shared launches (small circuits; every buffer above is cap times one proof's)
  int nbat = 0;   // proofs of the group in flight
  std::vector<uint8_t> rb, sb;  // blinding scalars of the proofs in flight, cap x 32 B each
  bool busy = false, collecting = false;
  // H in evaluation form (EvalTables): the proof in flight took that path; rows of its witness with a_j b_j != c_j, counted on the
  // device and copied to the pinned word before the sort of H (so it has landed when the proof's last chain has)
  bool eval = false;
  Dev<uint32_t> d_bad;
  Pinned<uint32_t> h_bad;
  std::vector<ProfSpan> spans;
  std::vector<ScopedEvent> event_pool;
  size_t event_next = 0;
};
}  // namespace zkr

namespace zkr {
// Side tables of the evaluation form (eval_h.hpp has the algebra), made from the scalars by a builder that knew them (zkr_setup.hip
// key_build_eval_tables) or from the key's own points for any whole key (zkr_eval_tables.hip zkr_key_eval_tables): the H
// multiexp over E' = -1/2 E with the coset products d_j as scalars, the C multiexp over C' = C + 1/2 C^T F.  Outside the arena: key
// files, replicas and contributed keys do not carry them and prove through the coefficient form until they are derived
// again; a shard gets its ranges of a whole key's tables when it is cut with ZKR_SHARD_SIDE_TABLES (zkr_multi.hip shard_eval_tables:
// E' over its range of the domain, C' over its point range, both with the shard's plans).  Both tables have the
// plans and the point layout of the tables they stand in for (C': the points of C, or of A's sort when the two share it, infinity
// where a scalar is zero; E': m points in natural order), so a proof uses the same sorts, bucket sets and chains either way.
struct EvalTables {
  bool ready = false;
  DevBuf c_pts, e_pts;
  Dev<uint32_t> c_rowptr, c_col, c_wide;  // C by QAP row, as the arena holds A and B, but with
  Dev<Fr> c_coef;                         // STANDARD-form coefficients: the row sums come out as c_j / R
  uint32_t n_wide = 0, nnz = 0;
  std::atomic<uint64_t> retries{0};  // proofs proved again through the coefficient form (their witness did not satisfy the R1CS)
};
int key_eval_tables_free(zkr_key *k);  // zkr_key.hip
bool eval_tables_alloc(zkr_key *k, uint32_t np_c, uint32_t np_e, uint32_t nnz, uint32_t n_wide);  // zkr_key.hip: room for all of them and the slots' counters; false: no memory
}  // namespace zkr

struct zkr_key {
  int device = 0;
  unsigned char *arena = nullptr;  // what every launch reads: arena_mem's block, or the caller's (zkr_key_adopt_arena), which is never freed here
  size_t arena_len = 0;
  zkr::Dev<unsigned char> arena_mem;
  zkr::Dev<unsigned char> base_arena;  // compact form for replication (zkr_key_base_arena), built on first request
  size_t base_arena_len = 0;
  zkr::ArenaHeader h;
  hipStream_t stream = nullptr;                    // the bucket accumulations
  zkr::WitnessStage stage[zkr::STAGE_BUFS];
  std::mutex stage_mu;
  std::condition_variable stage_freed;
  hipStream_t prep_stream = nullptr;               // digit records, digit sorts, calcH
  hipStream_t g2_stream = nullptr;                 // oversized buckets and reduction chain of the G2 table
  hipStream_t g1_stream = nullptr;                 // those of the G1 tables, one after the other
  hipStream_t aux_stream = nullptr;                // C's oversized-bucket partial sums in a lone proof of a small circuit, a shard's witness-side sorts
  void *streams_owner = nullptr;                   // the DeviceStreams set (zkr_key.hip) the stream handles above come from
  std::mutex *enqueue_mu = nullptr;                // the device's enqueue lock (shared streams: one proof's launches are enqueued without interleaving)
  zkr::ProofSlot slot[zkr::PROOF_SLOTS];
  int next_slot = 0;
  std::mutex mu;  // slot hand-out, the enqueue phase of a proof (so two host threads do not interleave launches), stage totals
  std::shared_mutex split_mu;  // a shard key: held EXCLUSIVELY by the sharded proof that splits calcH over it and its siblings (zkr_multi.hip
                               // run_sharded), SHARED by a shard proving on its own (zkr_prove_partial outside a split group)
  std::atomic<int> split_checked{0};  // a shard key: 0 = the split calcH has not been compared with the replicated form on this shard set yet
                                      // (or the comparison could not be made: it is tried again), 1 = compared, identical, 2 = it DISAGREED:
                                      // never split again (zkr_multi.hip run_sharded)
  int replica_mode = 0;        // how the key came to its device: 0 = loaded / built there, ZKR_REPLICATE_FULL / _BASE = zkr_key_replicate in that form
  bool replica_direct = false;  // ... and whether the two devices could address each other
  std::condition_variable slot_freed;
  zkr::MsmPlan plan[zkr::N_TABLES];
  zkr::ProofLayout layout;
  zkr::EvalTables eval;
  // proof assembly on the host: 4-bit window tables of delta_1 / delta_2 (built on first use)
  zkr::Dev<zkr::Tw29> tw29, twl29;  // butterfly twiddles, derived from the arena's tables when the key is set up (not part of the arena)
  std::once_flag delta_once;
  std::vector<zkr::G1Affine> delta1_tab;
  std::vector<zkr::G2Affine> delta2_tab;
  // profiling
  bool prof_on = false;
  std::vector<zkr::ProfStage> stages;
};

namespace zkr {
// every stream a proof of this key runs on idle (the streams are the device's: other keys' work on them is waited for too)
inline void key_streams_sync(zkr_key *k) {
  for (hipStream_t s : {k->stream, k->prep_stream, k->g2_stream, k->g1_stream, k->aux_stream}) (void)hipStreamSynchronize(s);
}
// zkr_key.hip
// What key_build makes a key from.  A table's source holds every point of its vector (affine Montgomery, 64 / 128 B per point);
// kept point j is source entry srcidx[j] and multiplies scalar sidx[j]
struct KeyTableSource {
  const void *src = nullptr;
  bool on_device = false;
  std::vector<uint32_t> srcidx, sidx;
};
struct KeySource {
  uint32_t n = 0, p = 0, m = 0;
  KeyRows side[2];  // A and B as the key holds them (qap_forms.hpp), Montgomery coefficients
  KeyTableSource tbl[N_TABLES];
  const uint8_t *consts448 = nullptr;  // alfa1 beta1 delta1 beta2 delta2 as the websnark header has them
};
int key_build(int device, const KeySource &src, zkr_key **out);
int key_alloc_workspace(zkr_key *k);
int fixed_base_points(int device, bool g2, const uint8_t *scalars_std, size_t n, DevBuf &out, bool wipe_scalars = false);  // out: device array of affine Montgomery points
int key_from_arena(int device, Dev<unsigned char> &&arena, const ArenaHeader &h, zkr_key **out);  // the key that owns `arena` from here on, with its workspace
// zkr_prove.hip
struct Prof {  // where a launch helper records its timing spans (null key: stage hooks, no timing)
  zkr_key *k;
  ProofSlot *sl;
};
constexpr Prof NO_PROF{nullptr, nullptr};
int prof_begin(Prof pf, hipStream_t s, const char *stage);
void prof_end(Prof pf, hipStream_t s, int span);
int prof_collect(zkr_key *k, ProofSlot &sl);
struct NttTables { const Fr *tw; const Tw29 *tw29, *twl29; int tlog; };  // x 2^256 powers of w_{2m} (coset factors); x 2^261 powers for the butterflies (kernels_ntt.hpp)
int ntt_lds_check(int device);  // ZKR_ERR_NO_DEVICE with a clear message when the device cannot hold an NTT tile in LDS
int ntt_tables29_build(const Fr *tw, uint32_t n_tw, const Fr *twl, uint32_t n_twl, hipStream_t s, Dev<Tw29> &tw29, Dev<Tw29> &twl29);
void ntt_twiddles_fill(Fr *tw, unsigned k, Fr *twl, hipStream_t s);  // tw[i] = w_{2^(k+1)}^i, 2^k entries; twl[i] = w_{2^(TWL_LOG+1)}^i, 2^TWL_LOG entries; launches only

// ShardGroup (the shards of one proof running concurrently; barrier + abort): shard_group.hpp, no HIP in it
// set by run_sharded's worker threads around zkr_prove_partial(_device): the proof this thread enqueues -- and collects -- is part
// `shard_group_part` of that group, which says whether calcH is split and whether H goes in evaluation form (null: a shard proving
// on its own -- replicated calcH, coefficient form)
extern thread_local ShardGroup *shard_group;
extern thread_local unsigned shard_group_part;
extern thread_local bool shard_turn_held;  // the caller of this thread's zkr_prove_partial(_device) holds the shard's split_mu already (run_sharded with a split calcH)
int fused_capacity(const ArenaHeader &h, const MsmPlan plan[N_TABLES]);
void arena_layout(ArenaHeader &h);  // section offsets and total_len from the sizes in the header (n, p, m, nnz, n_wide, npts, win_c, sc_n): THE layout, whoever builds an arena
const char *arena_header_fault(const ArenaHeader &h, size_t len);  // null when a full arena's header is consistent with its sizes
const char *window_fault(const ArenaHeader &h);  // null when the header's windows are ones the proof path can run with
void base_layout(const ArenaHeader &full, ArenaHeader &b);  // the same for the compact form (zkr_key_base_arena)
int arena_from_base(const void *dev_ptr, size_t len, int device, Dev<unsigned char> &arena_out, ArenaHeader *h_out);  // the full arena a compact one stands for, rebuilt
// zkr_prove.hip: sum_s scalars[s] * (table t of the key)[rank[s]] by the key's MSM path on a workspace of its own (zkr_key_contribution_verify);
// d_scalars: the table's whole scalar vector on the key's device, standard form below r; *out as the proof assembly reads MSM results
int key_table_msm(const zkr_key *k, int t, const Fr *d_scalars, XYZZ<Fq> *out);
// zkr_key_check.hip: what an arena whose header passed arena_header_fault CONTAINS (zkr_key_check; level 0 structure, 1 values)
int key_arena_check(int device, const unsigned char *arena, const ArenaHeader &h, int level, uint64_t report[4]);
// zkr_ptau.hip: the group elements of a key from a powers-of-tau transcript (zkr_setup_r1cs_ptau; delta = gamma = 1).
// cols: A (with the input-consistency rows), B, C over the domain m.  Steps 1-5 of zkr_ptau_verify run on the transcript first
// (ZKR_ERR_BAD_KEY).  d_tbl (device, Montgomery affine, infinity where a signal's polynomial vanishes):
// [T_A], [T_B1], [T_B2]: n points; [T_C]: the n points K[s] = beta A_s + alfa B_s + C_s (IC for s <= nPublic, C above); [T_H]: m
int ptau_key_tables(const void *ptau, size_t len, int device, uint32_t m, uint32_t n, const QapColumns cols[3], DevBuf d_tbl[N_TABLES], uint8_t consts448[448]);
// zkr_ptau.hip: its launches over vectors of G1 points, for the side tables derived from a key's own points (zkr_eval_tables.hip).
// On the current device and its null stream; points Montgomery affine x 2^256, x == 0 = infinity; ztmp: 2 n coordinates.
int g1_scale_each(G1Affine *pts, size_t n, const Fr *d_scalars, uint32_t sc_stride, void *ztmp);  // pts[i] <- s[i] pts[i]; scalars standard form, one per point (stride 1) or one for all (0)
int g1_group_ntt(G1Affine *pts, G1Affine *tmp, unsigned logn, bool inverse, Fr *tw, void *ztmp);  // natural order in and out, the inverse with 1 / n; tmp: n points, tw: n / 2 + 1 scalars
// out: point s < n = sum over column s of coefficient x pts[row]; partial sums lie behind
int g1_combine_columns(uint32_t n, const QapColumns &cols, const G1Affine *pts, DevBuf &out);
int device_bytes_equal(int device, const void *a, const void *b, size_t bytes, bool *same);  // zkr_contribute.hip: its compare kernel over one range; bytes a multiple of 16
int key_eval_rows(zkr_key *k, const Circuit &c);  // zkr_setup.hip: room for a whole key's side tables (eval_tables_alloc), C by row filled in; above zero: an allocation failed
int digit_lists_alloc(DigitLists &dl, size_t n_scalars, const MsmPlan &pl);
int msm_scratch_alloc(MsmScratch &m, size_t n_scalars, size_t n_points, const MsmPlan &pl, bool g2);  // for one proof of one table
int msm_precompute(int device, bool g2, void *d_table, uint32_t n, const MsmPlan &pl);  // fills levels 1..K-1 of a table whose level 0 is in place, then converts the table to the hot path's radix
int radix_convert(int device, bool g2, void *d_points, size_t count, bool to261);

// ---- what the audit of a finished key (zkr_key_audit.hip) takes from the other units
// zkr_ptau.hip: a verified transcript left on the device -- the body as Montgomery affine points, as ptau_upload leaves it -- with
// the byte offsets of its vectors in the host transcript
struct PtauOnDevice {
  unsigned power = 0;
  size_t M = 0;
  size_t off_tau1 = 0, off_tau2 = 0, off_alfa1 = 0, off_beta1 = 0, off_beta2 = 0;
  DevBuf body;
  const G1Affine *tau1 = nullptr, *alfa1 = nullptr, *beta1 = nullptr;  // 2 M, M, M points
  const G2Affine *tau2 = nullptr, *beta2 = nullptr;                    // M points, 1 point
};
const char *ptau_shape_fault(const void *ptau, size_t len, unsigned *power);  // null when header and length agree (step 1 of zkr_ptau_verify); host only
// zkr_ptau_verify itself; keep != null: the device form stays with the caller when the transcript verifies
int ptau_verify_keep(const void *ptau, size_t len, const uint8_t *records, size_t n_records, int device, int *valid, uint64_t rep[2], PtauOnDevice *keep);
// zkr_prove.hip: key_table_msm for the G2 table
int key_table_msm_g2(const zkr_key *k, const Fr *d_scalars, XYZZ<Fq2> *out);
// zkr_prove.hip: *same = the key's two twiddle sections are, byte for byte, the tables ntt_twiddles_fill makes for its domain (they
// are bytes of the key file otherwise: level 0 of zkr_key_check, which a load runs, does not look at them)
int key_twiddles_fresh_equal(const zkr_key *k, bool *same);
// zkr_prove.hip: nvec vectors of 2^logm words end to end, values on the domain -> coefficients: the prover's inverse transform
// with twiddle tables built FOR THIS CALL (nothing a key supplies), then natural order and the factor 1 / m; in: canonical,
// overwritten; out: nvec x m words; null stream, synchronised on return
int fresh_scalar_intt(int device, unsigned logm, Fr *d_in, Fr *d_out, int nvec);
// zkr_prove.hip: out[j] = sum_i scalars[j][i] pts[i], j < n_sums, over ONE vector of n finite points in device memory (Montgomery
// affine, left as it is): its window levels are built once, into a table that goes with the call, and every sum runs msm_enqueue
// over it with the identity rank map.  scalars: n words each, standard form below r.  out: n_sums XYZZ points of the group
int device_points_msm(int device, bool g2, const void *d_points, uint32_t n, const Fr *const *d_scalars, int n_sums, void *out_xyzz);
// zkr_r1cs.hip: the system as its kernels read it -- shape, the three CSR sides (0 A, 1 B, 2 C) on its device: row pointers
// (nC + 1), signals, Montgomery coefficients -- and the list of constraints with a side of more than wide_terms terms
struct R1csView {
  int device;
  uint32_t n, p, nC, m;
  const uint32_t *row_ptr[3], *col[3];
  const Fr *coef[3];
  const uint32_t *wide;
  uint32_t n_wide, wide_terms;
};
void r1cs_view(const zkr_r1cs *cs, R1csView *v);
}  // namespace zkr
