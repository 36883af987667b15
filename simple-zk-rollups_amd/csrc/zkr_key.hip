// zkr_key.hip -- proving-key ingestion: websnark binary -> device arena (CSR QAP rows, compacted
// Montgomery point tables, twiddle tables), replication hooks, workspace, fixed-base setup kernels.
//
// Replaces the key handling inside groth16GenProof (/root/reference/operator/src/snarks/common.ts:28-29);
// input layout is the one binarifyProvingKey writes (/root/reference/operator/src/utils/binarify.ts:143-206).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "kernels_msm.hpp"
#include "kernels_ntt.hpp"
#include "kernels_group.hpp"  // group_on_curve_launch for ZKR_CHECK_POINTS
#include "hostops.hpp"
#include <map>
#include "zkr_internal.hpp"

namespace zkr {

static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int os_random(void *out, size_t bytes) {
  static const char source[] = "/dev/urandom";
  FILE *f = fopen(source, "rb");
  if (!f) { set_error("cannot open %s", source); return ZKR_ERR_ARG; }
  const bool bad = fread(out, 1, bytes, f) != bytes;
  fclose(f);
  if (bad) { set_error("short read from %s", source); return ZKR_ERR_ARG; }
  return 0;
}

static inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// The arena's layout: header, twiddles, the two QAP sides (CSR), then per table its K window levels and its rank map.
// Everything that builds an arena -- key_build, the receiver of a compact arena, zkr_key_shard -- takes the offsets from here,
// so replicas and shards of one key agree byte for byte on where things are.
void arena_layout(ArenaHeader &h) {
  size_t off = ARENA_HEADER_BYTES;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return (uint64_t)o; };
  h.off_tw = take((size_t)h.m * 32);
  h.off_twl = take((size_t)(1u << TWL_LOG) * 32);
  for (int s = 0; s < 2; s++) {
    const uint32_t nnz = s == 0 ? h.nnzA : h.nnzB;
    h.off_rowptr[s] = take(((size_t)h.m + 1) * 4);
    h.off_col[s] = take((size_t)nnz * 4 + 4);
    h.off_coef[s] = take((size_t)nnz * 32 + 32);
    h.off_wide[s] = take((size_t)h.n_wide[s] * 4 + 4);
  }
  for (int t = 0; t < N_TABLES; t++) {
    const size_t pb = t == T_B2 ? 128 : 64, K = (255 + h.win_c[t] - 1) / h.win_c[t];
    h.off_pts[t] = take((size_t)h.npts[t] * K * pb + pb);  // K window levels per base point
    h.off_rank[t] = take((size_t)rank_entries(h, t) * 4 + 4);
  }
  h.total_len = off;
}

// Window bits of every table in 2..26, and ONE window for the four tables over the witness: its digit records are made once, with
// A's plan, and read by the sorts of B1, B2 and C with their own plans (zkr_prove.hip prove_submit_enqueue).  Keys built here always
// have it (msm_plan picks c from the scalar count, which the four share); a header that breaks it can still have a valid layout.
const char *window_fault(const ArenaHeader &h) {
  for (int t = 0; t < N_TABLES; t++)
    if (h.win_c[t] < 2 || h.win_c[t] > 26) return "bad window size";
  for (int t : {T_B1, T_B2, T_C})
    if (h.win_c[t] != h.win_c[T_A]) return "the tables A, B1, B2 and C share the witness's digit records but have different windows";
  return nullptr;
}

// A full arena's header against the layout its own sizes imply (arena_layout is the only producer): null when consistent, else
// what is wrong.  The sections' CONTENTS -- every index a kernel follows (row pointers, columns, wide rows, rank maps) -- are
// checked next, on the device, by key_arena_check (zkr_key_check.hip) before a loaded or adopted arena becomes a key: a damaged
// file or a foreign buffer is refused there, not found by a kernel reading past a section.
const char *arena_header_fault(const ArenaHeader &h, size_t len) {
  if (h.magic != ARENA_MAGIC) return "not a packed zkr key of this version (magic)";
  if (h.total_len != len) return "header total length differs from the bytes handed over";
  if (h.logm > 27 || h.m != (1u << h.logm) || h.n == 0 || h.p >= h.n) return "inconsistent circuit sizes";
  if (h.shard_parts < 1 || h.shard_parts > 64 || h.shard_part >= h.shard_parts) return "bad shard numbering";
  if (h.sc_n[0] > h.n || h.sc_lo[0] > h.n - h.sc_n[0] || h.sc_n[1] > h.m || h.sc_lo[1] > h.m - h.sc_n[1]) return "scalar ranges outside the vectors";
  if (h.shard_parts == 1 && (h.sc_lo[0] || h.sc_lo[1] || h.sc_n[0] != h.n || h.sc_n[1] != h.m)) return "a whole key whose scalar ranges are not the whole vectors";
  for (int s = 0; s < 2; s++)
    if (h.n_wide[s] > h.m) return "more wide rows than rows";
  if (const char *fault = window_fault(h)) return fault;
  for (int t = 0; t < N_TABLES; t++)
    if (h.npts[t] > rank_entries(h, t)) return "more points than scalars in a table";
  ArenaHeader want = h;
  arena_layout(want);
  bool same = want.total_len == h.total_len && want.off_tw == h.off_tw && want.off_twl == h.off_twl;
  for (int s = 0; s < 2; s++)
    same = same && want.off_rowptr[s] == h.off_rowptr[s] && want.off_col[s] == h.off_col[s] && want.off_coef[s] == h.off_coef[s] && want.off_wide[s] == h.off_wide[s];
  for (int t = 0; t < N_TABLES; t++) same = same && want.off_pts[t] == h.off_pts[t] && want.off_rank[t] == h.off_rank[t];
  return same ? nullptr : "section offsets differ from the layout the sizes imply";
}

// the sort buffers of a table of n points; cap: proofs a fused batch can hold (cap bucket sets end to end; kernels_msm.hpp
// msm_digits_count_kernel)
static int msm_sort_alloc(MsmSort &so, size_t n, const MsmPlan &pl, size_t cap) {
  size_t nb = pl.nb * cap;
  int rc;
  if ((rc = so.counts.alloc(nb + 1)) || (rc = so.offsets.alloc(nb + 1)) || (rc = so.size_hist.alloc(2 * SIZE_BINS)) || (rc = so.order.alloc(nb + 1)) ||
      (rc = so.chunk_cnt.alloc((size_t)pl.J * nb + 1)) || (rc = so.entries.alloc(n * pl.K * cap + 1)) || (rc = so.big_list.alloc(BIG_CAP)) ||
      (rc = so.big_count.alloc(4)) ||  // [0] oversized buckets, [1] total entries, [2] tile ticket (kernels_msm.hpp SortScratch)
      (rc = so.block_sums.alloc((nb / SCAN_BLOCK + 2) * 2)))  // the scan tiles' sums, 8 bytes each (msm_scan_sums_kernel, msm_scan_top_kernel)
    return rc;
  so.max_nb = nb;
  so.max_entries = n * pl.K * cap;
  return 0;
}
static size_t xyzz_bytes(bool g2) { return g2 ? sizeof(G2XYZZ) : sizeof(G1XYZZ); }
static int big_partials_alloc(DevBuf &p, bool g2) { return p.alloc((size_t)BIG_CAP * BIG_SPLIT * xyzz_bytes(g2)); }
// `sets` bucket sets per proof (2 in the chain that reduces A behind B1) of the plan's geometry, with their reduction buffers
static int msm_chain_alloc(MsmChain &ch, const MsmPlan &pl, bool g2, size_t cap, size_t sets) {
  const size_t nb = pl.nb * cap, xb = xyzz_bytes(g2);
  ch.sets = sets;
  ch.g2 = g2;
  int rc;
  if ((rc = ch.buckets.alloc(nb * sets * xb))) return rc;
  // sized for the plan's groups AND for the smaller groups of a latency-mode chain (zkr_prove.hip msm_reduce_enqueue: groups of
  // 2^LAT_GLOG buckets when nothing else is in flight), whose task sums take up to 16 splits
  const int g_min = pl.glog < LAT_GLOG ? pl.glog : LAT_GLOG;
  if ((rc = ch.group_out.alloc((size_t)(pl.nbw >> g_min) * cap * sets * 2 * xb)) ||
      (rc = ch.task_out.alloc((size_t)(pl.c + 2) * (pl.S > 16 ? pl.S : 16) * cap * sets * xb)) || (rc = ch.result.alloc(xb * cap * sets)))
    return rc;
  return ch.h_result.alloc(xb * cap * sets);
}
int digit_lists_alloc(DigitLists &dl, size_t n_scalars, const MsmPlan &pl) {  // n_scalars: of the whole (fused) vector
  int rc;
  if ((rc = dl.rng.alloc(DIGIT_RNG_WORDS)) || (rc = dl.ent_s.alloc((size_t)pl.K * n_scalars + 1))) return rc;
  return dl.ent_b.alloc((size_t)pl.K * n_scalars + 1);
}
// How many proofs of this key one submit fuses into shared launches: circuits far below the size that fills the chip
// (the reference's own tx circuit: 2^17) run every kernel over `cap` witnesses at once -- vectors end to end, `cap` bucket
// sets per table -- so each launch has about the work of one 2^20 proof and the fixed tail of the bucket reduction is
// paid once per batch.  Bounds: the batch's bucket ranges must fit the digit sort's MAX_RANGES lists, the fused vectors
// stay at or below 2^20 elements, at most 16.
int fused_capacity(const ArenaHeader &h, const MsmPlan plan[N_TABLES]) {
  if (h.shard_parts > 1) return 1;  // a shard multiplies a sub-range of one proof's vectors: nothing to lay end to end
  uint32_t nr = 1;
  for (int t = 0; t < N_TABLES; t++) nr = plan[t].nR > nr ? plan[t].nR : nr;
  uint32_t cap = MAX_RANGES / nr;
  uint32_t by_size = h.m >= (1u << 20) ? 1u : (1u << 20) / h.m;
  if (cap > by_size) cap = by_size;
  if (cap > (uint32_t)MAX_FUSE) cap = MAX_FUSE;
  return cap < 1 ? 1 : (int)cap;
}
int msm_scratch_alloc(MsmScratch &m, size_t n_scalars, size_t n, const MsmPlan &pl, bool g2) {
  int rc;
  if ((rc = digit_lists_alloc(m.dig, n_scalars, pl)) || (rc = msm_sort_alloc(m.sort, n, pl, 1)) || (rc = big_partials_alloc(m.big_partials, g2))) return rc;
  return msm_chain_alloc(m.chain, pl, g2, 1, 1);
}

// The streams of a device, made ONCE per process and shared by every key on that device.  The HIP runtime multiplexes the streams
// of one priority over GPU_MAX_HW_QUEUES = 4 hardware queues and hands the queues out as streams come and go: a process that had
// created and freed a few keys (the bench's replication leg; an operator with its tx and withdraw keys and a key cache) found two
// streams of its NEXT key on one hardware queue -- preparation and a reduction chain serialised, 10 % off every rate (tx circuit
// 940 against 1 040 proofs/s, the real circuit at 2^20 133 against 154; with GPU_MAX_HW_QUEUES=8 they came back:
// tools/bench_leg_interference*.sh).  One set per device never moves.  Two keys proving at the same time share the streams: the
// launches of one proof are enqueued under the device's enqueue lock, so every cross-stream wait points at work enqueued before it
// and the shared streams cannot wait for each other in a circle.
namespace {
struct DeviceStreams {
  hipStream_t accum = nullptr, prep = nullptr, g2 = nullptr, g1 = nullptr, aux = nullptr;  // zkr_internal.hpp zkr_key: the roles; raw and never destroyed, on purpose (above)
  std::mutex enqueue_mu;
};
std::mutex g_streams_mu;
std::map<int, DeviceStreams *> g_streams;  // never freed: the streams live as long as the process
}  // namespace

static int make_streams(DeviceStreams &ds) {
  // The accumulation stream is the bulk; preparation and reduction chains are short dependent launches whose
  // delay stalls it (the next sort, the proof's completion), so their workgroups are dispatched first.
  int prio_lo = 0, prio_hi = 0;
  ZKR_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));  // numerically lower = higher priority
  if (!ds.accum) ZKR_HIP_CHECK(hipStreamCreateWithPriority(&ds.accum, hipStreamNonBlocking, prio_lo));
  if (!ds.prep) ZKR_HIP_CHECK(hipStreamCreateWithPriority(&ds.prep, hipStreamNonBlocking, prio_hi));
  if (!ds.g2) ZKR_HIP_CHECK(hipStreamCreateWithPriority(&ds.g2, hipStreamNonBlocking, prio_hi));
  if (!ds.g1) ZKR_HIP_CHECK(hipStreamCreateWithPriority(&ds.g1, hipStreamNonBlocking, prio_hi));
  // one more for C's oversized-bucket sums in a lone proof of a small circuit, and for a shard's witness-side sorts.  At the MIDDLE priority: a fifth
  // high-priority stream made the next one created -- the witness builder's (rollup_gpu.hip) -- share a hardware queue with the
  // preparation stream: its 28 ms kernel then stalled every proof behind it (facade pipeline 623 against 840 batches/s, tools/ab_hw_queues2.sh)
  if (!ds.aux) ZKR_HIP_CHECK(hipStreamCreateWithPriority(&ds.aux, hipStreamNonBlocking, (prio_lo + prio_hi) / 2));
  return 0;
}

int key_alloc_workspace(zkr_key *k) {
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  if (int lrc = ntt_lds_check(k->device)) return lrc;
  const ArenaHeader &h = k->h;
  // reduction streams: the chains of one proof add up to ~6 ms of serialised launches, so on a single in-order
  // stream they, not the accumulations, set the pace with two proofs in flight (94 vs 106 proofs/s with two)
  for (int t = 0; t < N_TABLES; t++) k->plan[t] = msm_plan(rank_entries(h, t), h.npts[t], (int)h.win_c[t]);
  k->layout = proof_layout(h.npts, h.share_b != 0, h.share_ac != 0, k->plan);
  const ProofLayout &lay = k->layout;
  // Two reduction streams: the G2 chain on one, the G1 chains one after the other on the other.  Round 2 ran circuits that fill the
  // chip alone with three (136.3 against 132.1 proofs/s at 2^20); since C and H share one chain and the G2 reductions take a
  // whole SIMD's registers, the third stream only adds contention for the accumulations: 152.5-153.5 against 145.9-146.6
  // proofs/s at 2^20 (three same-box rounds), 38.5 against 37.4 at 2^22, a synchronous 2^20 proof 7.75 against 8.0 ms; one
  // stream: 122 (tools/sweep_knobs2.sh).  Keys whose proofs are fused into shared launches always ran with two (fewer, fatter
  // chains: 2^16 1745 against 1680, 2^17 943 against 910, 2^18 514 against 492, 2^19 237 against 231, the tx circuit 988
  // against 957 proofs/s).
  {
    DeviceStreams *ds = nullptr;
    {
      std::lock_guard<std::mutex> lk(g_streams_mu);
      DeviceStreams *&slot = g_streams[k->device];
      if (!slot) slot = new DeviceStreams();
      ds = slot;
    }
    int src = 0;
    {
      std::lock_guard<std::mutex> lk(g_streams_mu);  // creation of missing streams of a shared set, one key at a time
      src = make_streams(*ds);
    }
    if (src) return src;
    k->streams_owner = ds;
    k->enqueue_mu = &ds->enqueue_mu;
    k->stream = ds->accum;
    k->prep_stream = ds->prep;
    k->g2_stream = ds->g2;
    k->g1_stream = ds->g1;
    k->aux_stream = ds->aux;
  }
  {
    int rc = ntt_tables29_build((const Fr *)(k->arena + h.off_tw), 1u << h.tlog, (const Fr *)(k->arena + h.off_twl), 1u << TWL_LOG, nullptr, k->tw29, k->twl29);
    if (rc) return rc;
  }
  const size_t cap = (size_t)fused_capacity(h, k->plan);
  for (ProofSlot &sl : k->slot) {
    sl.cap = (int)cap;
    sl.rb.assign(32 * cap, 0);
    sl.sb.assign(32 * cap, 0);
    int rc = 0;
    for (ScopedEvent *e : {sl.ev_done, sl.ev_sorted, sl.ev_res})
      for (int t = 0; t < N_TABLES && !rc; t++) rc = e[t].create(hipEventDisableTiming);
    for (ScopedEvent *e : {&sl.ev_w, &sl.ev_h, &sl.ev_end[0], &sl.ev_end[1], &sl.ev_end[2]})
      if (!rc) rc = e->create(hipEventDisableTiming);
    if (!rc) rc = sl.d_w.alloc((size_t)h.n * cap);
    for (Dev<Fr> *v : {&sl.va, &sl.vb, &sl.ca, &sl.cb, &sl.d_h})
      if (!rc) rc = v->alloc((size_t)h.m * cap);
    for (int t = 0; t < N_TABLES && !rc; t++) {
      if (!h.npts[t]) continue;  // an empty table is sorted, accumulated and reduced nowhere (it is in no chain of the layout)
      if (lay.sort_src[t] == t) rc = msm_sort_alloc(sl.sort[t], h.npts[t], k->plan[t], cap);
      if (!rc) rc = big_partials_alloc(sl.big_partials[t], t == T_B2);
    }
    for (int c = 0; c < lay.n_chains && !rc; c++) rc = msm_chain_alloc(sl.chain[c], k->plan[lay.chains[c].geom], lay.chains[c].g2, cap, (size_t)lay.chains[c].sets);
    if (!rc) rc = digit_lists_alloc(sl.dig_w, (size_t)h.sc_n[0] * cap, k->plan[T_A]);
    if (!rc) rc = digit_lists_alloc(sl.dig_h, (size_t)h.sc_n[1] * cap, k->plan[T_H]);
    if (rc) return rc;
  }
  // host-side window tables of delta_1 / delta_2 for the proof assembly (a few milliseconds; kept out of the first proof)
  std::call_once(k->delta_once, [&] {
    k->delta1_tab = fixed_base_table(load_g1(h.delta1));
    k->delta2_tab = fixed_base_table(load_g2(h.delta2));
  });
  return 0;
}

// Room for the side tables of the evaluation form, whoever fills them: C' of np_c points and E' of np_e with the key's plans of C
// and H (sized as arena_layout sizes a table), C by row (nnz terms, n_wide wide rows) over the whole domain, and per proof slot a
// counter for each proof of a fused group, device and pinned, the pinned ones zero.  False: the device or the host has no memory
// for them -- what is allocated stays until key_eval_tables_free, and what follows is the caller's policy.
bool eval_tables_alloc(zkr_key *k, uint32_t np_c, uint32_t np_e, uint32_t nnz, uint32_t n_wide) {
  EvalTables &ev = k->eval;
  ev.nnz = nnz;
  ev.n_wide = n_wide;
  bool ok = !ev.c_pts.alloc((size_t)np_c * k->plan[T_C].K * 64 + 64) && !ev.e_pts.alloc((size_t)np_e * k->plan[T_H].K * 64 + 64) &&
            !ev.c_rowptr.alloc((size_t)k->h.m + 1) && !ev.c_col.alloc((size_t)nnz + 1) && !ev.c_coef.alloc((size_t)nnz + 1) && !ev.c_wide.alloc((size_t)n_wide + 1);
  for (ProofSlot &sl : k->slot) {
    ok = ok && !sl.d_bad.alloc((size_t)sl.cap) && !sl.h_bad.alloc((size_t)sl.cap);
    if (ok) memset(sl.h_bad, 0, (size_t)sl.cap * 4);
  }
  return ok;
}

// the side tables of the evaluation form and what the slots hold for them; the key's proofs must have been collected
int key_eval_tables_free(zkr_key *k) {
  EvalTables &ev = k->eval;
  ev.ready = false;
  ev.c_pts.reset(); ev.e_pts.reset(); ev.c_rowptr.reset(); ev.c_col.reset(); ev.c_coef.reset(); ev.c_wide.reset();
  for (ProofSlot &sl : k->slot) { sl.d_bad.reset(); sl.h_bad.reset(); }
  return 0;
}

// `count` affine points between the key's Montgomery radix (2^256) and the hot path's (2^261), in place
int radix_convert(int device, bool g2, void *d_points, size_t count, bool to261) {
  if (count == 0) return 0;
  ZKR_HIP_CHECK(hipSetDevice(device));
  unsigned grid = (unsigned)((count + MSM_THREADS - 1) / MSM_THREADS);
  if (g2) radix_convert_kernel<Fq2><<<grid, MSM_THREADS>>>((G2Affine *)d_points, count, to261 ? 1 : 0);
  else radix_convert_kernel<Fq><<<grid, MSM_THREADS>>>((G1Affine *)d_points, count, to261 ? 1 : 0);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipDeviceSynchronize());
  return 0;
}

// Level 0 of the table (n points, the key's wire form: coordinates x 2^256) is in place: fills levels 1..K-1 and rewrites
// level 0, all in the radix of the accumulation kernels (x 2^261, canonical; kernels_msm.hpp header).
// ZKR_CHECK_POINTS=1: every base point of a table (wire form, x 2^256) satisfies its curve's equation y^2 = x^3 + b before
// anything is derived from it.  Off by default, as in the reference (websnark multiplies whatever the key holds): a point off
// the curve makes the window-table build produce garbage multiples silently (its doubling chain may hit Y = 0).
static int check_points_on_curve(bool g2, const void *d_table, uint32_t n) {
  FaultCounter bad;
  int rc;
  if ((rc = bad.reset())) return rc;
  if (g2) group_on_curve_launch<Fq2>(d_table, n, true, bad.dev());  // infinity passes: the placeholder of a shared-support table
  else group_on_curve_launch<Fq>(d_table, n, true, bad.dev());
  if ((rc = bad.read())) return rc;
  if (bad.count) {
    set_error("%u point(s) of a %s table are not on the curve (first: kept point %u); ZKR_CHECK_POINTS=1", bad.count, g2 ? "G2" : "G1", bad.first);
    return ZKR_ERR_BAD_KEY;
  }
  return 0;
}

int msm_precompute(int device, bool g2, void *d_table, uint32_t n, const MsmPlan &pl) {
  if (n == 0) return 0;
  ZKR_HIP_CHECK(hipSetDevice(device));
  if (const char *e = getenv("ZKR_CHECK_POINTS"); e && atoi(e) != 0)
    if (int crc = check_points_on_curve(g2, d_table, n)) return crc;
  if (pl.K < 2) return radix_convert(device, g2, d_table, (size_t)n, true);
  const int levels = pl.K - 1 < PRE_LEVELS ? pl.K - 1 : PRE_LEVELS;
  DevBuf zbuf;  // denominators of one chunk of levels (msm_precompute_kernel)
  if (int arc = zbuf.alloc((size_t)n * levels * (g2 ? sizeof(Fq2) : sizeof(Fq)))) return arc;
  void *ztmp = zbuf.p;
  unsigned grid = (n + MSM_THREADS - 1) / MSM_THREADS;
  if (g2) msm_precompute_kernel<Fq2, 1><<<grid, MSM_THREADS>>>((G2Affine *)d_table, n, pl.c, pl.K, (Fq2 *)ztmp);
  else msm_precompute_kernel<Fq, 2><<<grid, MSM_THREADS>>>((G1Affine *)d_table, n, pl.c, pl.K, (Fq *)ztmp);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("window-table build failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  return 0;
}

// the key over an arena this library allocated: it owns the block from here on, whether or not its workspace can be made
int key_from_arena(int device, Dev<unsigned char> &&arena, const ArenaHeader &h, zkr_key **out) {
  zkr_key *k = new zkr_key();
  k->device = device;
  k->arena_mem = std::move(arena);
  k->arena = k->arena_mem;
  k->arena_len = h.total_len;
  k->h = h;
  int rc = key_alloc_workspace(k);
  if (rc) { zkr_key_free(k); return rc; }
  *out = k;
  return 0;
}

// Builds the arena from the rows and the kept points of `ks` (zkr_internal.hpp KeySource).
int key_build(int device, const KeySource &ks, zkr_key **out) {
  const uint32_t n = ks.n, m = ks.m;
  ZKR_HIP_CHECK(hipSetDevice(device));
  ArenaHeader h;
  memset(&h, 0, sizeof(h));
  h.magic = ARENA_MAGIC;
  h.n = n; h.p = ks.p; h.m = m;
  h.logm = domain_log2(m);
  h.tlog = h.logm;
  h.nnzA = (uint32_t)ks.side[0].col.size();
  h.nnzB = (uint32_t)ks.side[1].col.size();
  header_set_consts(h, ks.consts448);
  h.sc_lo[0] = h.sc_lo[1] = 0; h.sc_n[0] = n; h.sc_n[1] = m;
  h.shard_part = 0; h.shard_parts = 1;
  std::vector<uint32_t> wide[2];
  for (int s = 0; s < 2; s++) {
    wide[s] = wide_rows(ks.side[s].rowptr.data(), m);
    h.n_wide[s] = (uint32_t)wide[s].size();
  }
  // A and C multiply the same scalars and nearly the same signals (C lacks the public ones): when their supports
  // overlap by >= 90 % both tables are laid out over the UNION of the supports (a missing point is stored as
  // infinity, x = 0, and skipped by the accumulation), so one digit sort serves both (h.share_ac).
  const std::vector<uint32_t> *srcidx_eff[N_TABLES], *sidx_eff[N_TABLES];
  for (int t = 0; t < N_TABLES; t++) { srcidx_eff[t] = &ks.tbl[t].srcidx; sidx_eff[t] = &ks.tbl[t].sidx; }
  std::vector<uint32_t> u_sidx, uA_src, uC_src;
  {
    const std::vector<uint32_t> &sa = ks.tbl[T_A].sidx, &sc = ks.tbl[T_C].sidx;
    size_t i = 0, j = 0, both = 0;
    while (i < sa.size() || j < sc.size()) {
      uint32_t a = i < sa.size() ? sa[i] : 0xffffffffu, c = j < sc.size() ? sc[j] : 0xffffffffu;
      uint32_t s = a < c ? a : c;
      u_sidx.push_back(s);
      uA_src.push_back(a == s ? ks.tbl[T_A].srcidx[i] : RANK_NONE);
      uC_src.push_back(c == s ? ks.tbl[T_C].srcidx[j] : RANK_NONE);
      both += (a == s && c == s);
      if (a == s) i++;
      if (c == s) j++;
    }
    if (!u_sidx.empty() && both * 10 >= u_sidx.size() * 9) {
      h.share_ac = 1;
      srcidx_eff[T_A] = &uA_src; srcidx_eff[T_C] = &uC_src;
      sidx_eff[T_A] = sidx_eff[T_C] = &u_sidx;
    }
  }
  MsmPlan plan[N_TABLES];
  for (int t = 0; t < N_TABLES; t++) {
    h.npts[t] = (uint32_t)srcidx_eff[t]->size();
    plan[t] = msm_plan(t == T_H ? m : n, h.npts[t]);
    h.win_c[t] = (uint32_t)plan[t].c;
  }
  h.share_b = ks.tbl[T_B1].sidx == ks.tbl[T_B2].sidx ? 1 : 0;
  arena_layout(h);
  const size_t off = h.total_len;

  Dev<unsigned char> arena;
  if (int arc = arena.alloc(off)) return arc;
  ZKR_HIP_CHECK(hipMemset(arena, 0, off));  // alignment gaps and slack bytes are part of the arena's bytes (replicas, packed key files): defined, not stale
  ZKR_HIP_CHECK(hipMemcpy(arena, &h, sizeof(h), hipMemcpyHostToDevice));
  for (int s = 0; s < 2; s++) {
    const KeyRows &q = ks.side[s];
    ZKR_HIP_CHECK(hipMemcpy(arena + h.off_rowptr[s], q.rowptr.data(), q.rowptr.size() * 4, hipMemcpyHostToDevice));
    if (!q.col.empty()) {
      ZKR_HIP_CHECK(hipMemcpy(arena + h.off_col[s], q.col.data(), q.col.size() * 4, hipMemcpyHostToDevice));
      ZKR_HIP_CHECK(hipMemcpy(arena + h.off_coef[s], q.coef.data(), q.coef.size(), hipMemcpyHostToDevice));
    }
    if (!wide[s].empty()) ZKR_HIP_CHECK(hipMemcpy(arena + h.off_wide[s], wide[s].data(), wide[s].size() * 4, hipMemcpyHostToDevice));
  }
  for (int t = 0; t < N_TABLES; t++) {
    size_t np = h.npts[t], pb = t == T_B2 ? 128 : 64;
    if (!np) continue;
    {  // scalar index -> point index (RANK_NONE: the key has the point at infinity there)
      std::vector<uint32_t> rank(t == T_H ? m : n, RANK_NONE);
      for (size_t j = 0; j < np; j++) rank[(*sidx_eff[t])[j]] = (uint32_t)j;
      bool ident = np == rank.size();
      for (size_t j = 0; ident && j < np; j++) ident = rank[j] == (uint32_t)j;
      h.rank_identity[t] = ident ? 1 : 0;
      ZKR_HIP_CHECK(hipMemcpy(arena + h.off_rank[t], rank.data(), rank.size() * 4, hipMemcpyHostToDevice));
    }
    if (ks.tbl[t].on_device) {
      Dev<uint32_t> d_idx;
      if (int irc = d_idx.alloc(np)) return irc;
      ZKR_HIP_CHECK(hipMemcpy(d_idx, srcidx_eff[t]->data(), np * 4, hipMemcpyHostToDevice));
      unsigned grid = (unsigned)((np * (pb / 16) + 255) / 256);  // one 16-byte piece per thread
      if (t == T_B2)
        gather_kernel<G2Affine><<<grid, 256>>>((const G2Affine *)ks.tbl[t].src, d_idx, np, (G2Affine *)(arena + h.off_pts[t]));
      else
        gather_kernel<G1Affine><<<grid, 256>>>((const G1Affine *)ks.tbl[t].src, d_idx, np, (G1Affine *)(arena + h.off_pts[t]));
      ZKR_HIP_CHECK(hipGetLastError());
      ZKR_HIP_CHECK(hipDeviceSynchronize());
    } else {
      std::vector<uint8_t> stage(np * pb);
      const uint8_t *src = (const uint8_t *)ks.tbl[t].src;
      for (size_t j = 0; j < np; j++) {
        uint32_t si = (*srcidx_eff[t])[j];
        if (si != RANK_NONE) memcpy(&stage[j * pb], src + (size_t)si * pb, pb);  // else: stays all-zero = infinity (x = 0)
      }
      ZKR_HIP_CHECK(hipMemcpy(arena + h.off_pts[t], stage.data(), np * pb, hipMemcpyHostToDevice));
    }
    if (int rc = msm_precompute(device, t == T_B2, arena + h.off_pts[t], (uint32_t)np, plan[t])) return rc;
  }
  ZKR_HIP_CHECK(hipMemcpy(arena, &h, sizeof(h), hipMemcpyHostToDevice));  // again: rank_identity was filled in above
  // twiddles on device: T[k] = w_{2m}^k and w_2048^k
  ntt_twiddles_fill((Fr *)(arena + h.off_tw), h.logm, (Fr *)(arena + h.off_twl), nullptr);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipDeviceSynchronize());

  return key_from_arena(device, std::move(arena), h, out);
}

// scalars (host, std form) * generator -> device array of affine Montgomery points in `out`.  wipe: the
// scalars are secret (setup with fresh toxic waste): their device copy is zeroed before it is freed, on every path.
template <class F>
static int fixed_base_impl(int device, const Affine<F> &gen, const uint8_t *scalars_std, size_t n, DevBuf &out, bool wipe) {
  ZKR_HIP_CHECK(hipSetDevice(device));
  // T[j][d] = d * 2^(8j) * G on the host (8160 group operations, once per generator)
  std::vector<Affine<F>> table(32 * 256);
  XYZZ<F> base = to_xyzz(gen);
  for (int j = 0; j < 32; j++) {
    XYZZ<F> cur = XYZZ<F>::inf();
    for (int d = 1; d < 256; d++) {
      cur = add_full(cur, base);
      table[j * 256 + d] = to_affine(cur);
    }
    table[j * 256] = Affine<F>{F::zero(), F::one()};
    for (int b = 0; b < 8; b++) base = dbl_xyzz(base);
  }
  struct Scalars {  // their device copy, cleared before it is freed when they are secret, however the function is left
    Dev<Fr> sc;
    size_t bytes = 0;
    bool wipe = false;
    ~Scalars() {
      if (sc && wipe) { hipMemset(sc, 0, bytes); hipDeviceSynchronize(); }
    }
  } d;
  d.wipe = wipe;
  d.bytes = (n + 1) * 32;
  Dev<Affine<F>> d_table, pts;
  int rc;
  if ((rc = d_table.alloc(table.size())) || (rc = pts.alloc(n + 1)) || (rc = d.sc.alloc(n + 1))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(d_table, table.data(), table.size() * sizeof(Affine<F>), hipMemcpyHostToDevice));
  ZKR_HIP_CHECK(hipMemcpy(d.sc, scalars_std, n * 32, hipMemcpyHostToDevice));
  constexpr int MINW = sizeof(F) == 32 ? 2 : 1;
  fixed_base_kernel<F, MINW><<<(unsigned)((n + 255) / 256), 256>>>(d_table, d.sc, n, pts);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipDeviceSynchronize());
  out = std::move(pts.buf);
  return 0;
}

int fixed_base_points(int device, bool g2, const uint8_t *scalars_std, size_t n, DevBuf &out, bool wipe_scalars) {
  if (!g2) {
    G1Affine g{Fq::one(), add(Fq::one(), Fq::one())};  // (1, 2), TxVerifier.sol:24-26
    return fixed_base_impl<Fq>(device, g, scalars_std, n, out, wipe_scalars);
  }
  const G2Affine g = g2_generator();
  return fixed_base_impl<Fq2>(device, g, scalars_std, n, out, wipe_scalars);
}

}  // namespace zkr

using namespace zkr;

extern "C" {

const char *zkr_last_error(void) { return g_err; }
const char *zkr_version(void) { return "zkr-hip 0.1 (gfx950)"; }

int zkr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int zkr_device_pci_bus_id(int device, char *out, size_t out_len) {
  if (!out || out_len < 16) { set_error("buffer too small"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipDeviceGetPCIBusId(out, (int)out_len, device));
  return 0;
}

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static bool all_zero(const uint8_t *p, size_t n) { for (size_t i = 0; i < n; i++) if (p[i]) return false; return true; }

int zkr_key_load_websnark(const void *pk_bin, size_t pk_len, int device, zkr_key **out) {
  if (!pk_bin || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  const uint8_t *pk = (const uint8_t *)pk_bin;
  if (pk_len < 488) { set_error("proving key shorter than its fixed header (488 bytes)"); return ZKR_ERR_BAD_KEY; }
  uint32_t n = rd32(pk), p = rd32(pk + 4), m = rd32(pk + 8);
  uint32_t ptr[7];
  for (int i = 0; i < 7; i++) ptr[i] = rd32(pk + 12 + 4 * i);
  if (n == 0 || (uint64_t)p + 1 > n || m < 2 || (m & (m - 1))) { set_error("bad key geometry nVars=%u nPublic=%u domainSize=%u", n, p, m); return ZKR_ERR_BAD_KEY; }
  if (ptr[0] != 488) { set_error("polsA pointer %u != 488", ptr[0]); return ZKR_ERR_BAD_KEY; }
  // the two pols sections are scanned before anything else: their bounds must lie inside the caller's buffer
  if ((uint64_t)ptr[1] < 488 || (uint64_t)ptr[1] > (uint64_t)ptr[2] || (uint64_t)ptr[2] > (uint64_t)pk_len) {
    set_error("pols pointers out of order or past the buffer (polsB %u, pointsA %u, length %zu)", ptr[1], ptr[2], pk_len);
    return ZKR_ERR_BAD_KEY;
  }
  // point sections have fixed sizes (binarify.ts:129-138)
  uint64_t expect_end = (uint64_t)ptr[2] + 64ull * n + 64ull * n + 128ull * n + 64ull * (n - p - 1) + 64ull * m;
  if (ptr[3] != ptr[2] + 64ull * n || ptr[4] != ptr[3] + 64ull * n || ptr[5] != ptr[4] + 128ull * n || ptr[6] != ptr[5] + 64ull * (n - p - 1) ||
      expect_end != pk_len) {
    set_error("section pointers/length inconsistent with nVars=%u nPublic=%u domainSize=%u (len %zu)", n, p, m, pk_len);
    return ZKR_ERR_BAD_KEY;
  }
  KeySource ks;
  ks.n = n; ks.p = p; ks.m = m;
  ks.consts448 = pk + 40;
  for (int s = 0; s < 2; s++)
    if (int rc = pols_to_rows(pk, ptr[s], ptr[s + 1], s, n, m, ks.side[s])) return rc;
  // point tables: drop points at infinity (x == 0), remember which scalar each kept point multiplies
  for (int t = 0; t < N_TABLES; t++) ks.tbl[t].src = pk + ptr[2 + t];
  auto keep = [&](int t, uint32_t src, uint32_t scalar) { ks.tbl[t].srcidx.push_back(src); ks.tbl[t].sidx.push_back(scalar); };
  for (uint32_t i = 0; i < n; i++) {
    if (!all_zero(pk + ptr[2] + 64ull * i, 32)) keep(T_A, i, i);
    if (!all_zero(pk + ptr[3] + 64ull * i, 32)) keep(T_B1, i, i);
    if (!all_zero(pk + ptr[4] + 128ull * i, 64)) keep(T_B2, i, i);
  }
  for (uint32_t i = 0; i + p + 1 < n; i++)
    if (!all_zero(pk + ptr[5] + 64ull * i, 32)) keep(T_C, i, i + p + 1);
  const unsigned logm = domain_log2(m);
  for (uint32_t j = 0; j < m; j++) {  // h is produced in bit-reversed order: pair position j with hExps[bitrev(j)]
    const uint32_t i = bitrev32(j, logm);
    if (!all_zero(pk + ptr[6] + 64ull * i, 32)) keep(T_H, i, j);
  }
  return key_build(device, ks, out);
}

void zkr_key_free(zkr_key *k) {
  if (!k) return;
  hipSetDevice(k->device);
  // the streams are the device's (one set per device, shared by its keys): wait for THIS key's work only -- the last events of its
  // proof slots and staged uploads (an event that was never recorded is complete) -- not for the proofs other keys have in flight
  for (ProofSlot &sl : k->slot) {
    for (hipEvent_t e : sl.ev_end)
      if (e) hipEventSynchronize(e);
    for (int t = 0; t < N_TABLES; t++)
      if (sl.ev_res[t]) hipEventSynchronize(sl.ev_res[t]);
  }
  for (WitnessStage &ws : k->stage)
    if (ws.ev_up) hipEventSynchronize(ws.ev_up);
  delete k;  // every buffer, event and table goes with its owner; a caller's arena (zkr_key_adopt_arena) is not among them
}

int zkr_key_info(const zkr_key *k, uint64_t out[10]) {
  if (!k || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  out[0] = k->h.n; out[1] = k->h.p; out[2] = k->h.m; out[3] = k->h.nnzA; out[4] = k->h.nnzB;
  for (int t = 0; t < N_TABLES; t++) out[5 + t] = k->h.npts[t];
  return 0;
}

int zkr_key_h_form(const zkr_key *k, int *evaluation, uint64_t *retries) {
  if (!k) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (evaluation) *evaluation = k->eval.ready ? 1 : 0;
  if (retries) *retries = k->eval.retries.load();
  return 0;
}

int zkr_key_slots(const zkr_key *k) { return k ? PROOF_SLOTS : 0; }
int zkr_key_fuse(const zkr_key *k) { return k ? k->slot[0].cap : 0; }

int zkr_key_windows(const zkr_key *k, uint32_t c_out[5], uint32_t k_out[5]) {
  if (!k || !c_out || !k_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  for (int t = 0; t < N_TABLES; t++) { c_out[t] = (uint32_t)k->plan[t].c; k_out[t] = (uint32_t)k->plan[t].K; }
  return 0;
}

int zkr_key_arena(const zkr_key *k, void **dev_ptr, size_t *len) {
  if (!k || !dev_ptr || !len) { set_error("null argument"); return ZKR_ERR_ARG; }
  *dev_ptr = k->arena;
  *len = k->arena_len;
  return 0;
}

int zkr_key_adopt_arena(void *dev_ptr, size_t len, int device, zkr_key **out) {
  if (!dev_ptr || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  ArenaHeader h;
  if (len < ARENA_HEADER_BYTES) { set_error("arena too small"); return ZKR_ERR_BAD_KEY; }
  ZKR_HIP_CHECK(hipMemcpy(&h, dev_ptr, sizeof(h), hipMemcpyDeviceToHost));
  if (const char *fault = arena_header_fault(h, len)) { set_error("arena header: %s", fault); return ZKR_ERR_BAD_KEY; }
  if (int rc = key_arena_check(device, (const unsigned char *)dev_ptr, h, 0, nullptr)) return rc;
  zkr_key *k = new zkr_key();
  k->device = device;
  k->arena = (unsigned char *)dev_ptr;  // the caller's: arena_mem stays empty
  k->arena_len = len;
  k->h = h;
  int rc = key_alloc_workspace(k);
  if (rc) { zkr_key_free(k); return rc; }
  *out = k;
  return 0;
}

// ---- compact form of the arena for replication over slow links: header + CSR rows + LEVEL 0 of every
// point table + rank maps; the window levels 1..K-1 (12/13 of the arena) and the twiddle tables are rebuilt by the
// receiver (msm_precompute_kernel, twiddle_table_kernel).  Same ArenaHeader with BASE_MAGIC and offsets of the compact
// layout; win_c / npts / share flags carry over so the rebuilt arena is byte-identical to the sender's.
constexpr uint64_t BASE_MAGIC = 0x32304245534b525aull;  // "ZRKSEB02"-ish tag: distinct from ARENA_MAGIC

}  // extern "C"
namespace zkr {
void base_layout(const ArenaHeader &full, ArenaHeader &b) {
  b = full;
  b.magic = BASE_MAGIC;
  size_t off = ARENA_HEADER_BYTES;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return (uint64_t)o; };
  b.off_tw = b.off_twl = 0;
  for (int s = 0; s < 2; s++) {
    uint32_t nnz = s == 0 ? full.nnzA : full.nnzB;
    b.off_rowptr[s] = take(((size_t)full.m + 1) * 4);
    b.off_col[s] = take((size_t)nnz * 4 + 4);
    b.off_coef[s] = take((size_t)nnz * 32 + 32);
    b.off_wide[s] = take((size_t)full.n_wide[s] * 4 + 4);
  }
  for (int t = 0; t < N_TABLES; t++) {
    size_t pb = t == T_B2 ? 128 : 64;
    b.off_pts[t] = take((size_t)full.npts[t] * pb + pb);
    b.off_rank[t] = take((size_t)rank_entries(full, t) * 4 + 4);
  }
  b.total_len = off;
}
}  // namespace zkr
extern "C" {

int zkr_key_base_arena(zkr_key *k, void **dev_ptr, size_t *len) {
  if (!k || !dev_ptr || !len) { set_error("null argument"); return ZKR_ERR_ARG; }
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  std::lock_guard<std::mutex> lk(k->mu);
  if (!k->base_arena) {
    ArenaHeader b;
    base_layout(k->h, b);
    Dev<unsigned char> buf;
    if (int arc = buf.alloc(b.total_len)) return arc;
    auto cp = [&](uint64_t dst, uint64_t src, size_t bytes) { return bytes ? hipMemcpy(buf + dst, k->arena + src, bytes, hipMemcpyDeviceToDevice) : hipSuccess; };
    hipError_t e = hipMemset(buf, 0, b.total_len);
    if (e == hipSuccess) e = hipMemcpy(buf, &b, sizeof(b), hipMemcpyHostToDevice);
    for (int s = 0; s < 2 && e == hipSuccess; s++) {
      uint32_t nnz = s == 0 ? k->h.nnzA : k->h.nnzB;
      e = cp(b.off_rowptr[s], k->h.off_rowptr[s], ((size_t)k->h.m + 1) * 4);
      if (e == hipSuccess) e = cp(b.off_col[s], k->h.off_col[s], (size_t)nnz * 4);
      if (e == hipSuccess) e = cp(b.off_coef[s], k->h.off_coef[s], (size_t)nnz * 32);
      if (e == hipSuccess) e = cp(b.off_wide[s], k->h.off_wide[s], (size_t)k->h.n_wide[s] * 4);
    }
    for (int t = 0; t < N_TABLES && e == hipSuccess; t++) {
      e = cp(b.off_pts[t], k->h.off_pts[t], (size_t)k->h.npts[t] * (t == T_B2 ? 128 : 64));
      if (e == hipSuccess) e = cp(b.off_rank[t], k->h.off_rank[t], (size_t)rank_entries(k->h, t) * 4);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("building the compact arena failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
    // the compact form carries the base points in the key's own radix (2^256): the receiver rebuilds the window levels from
    // them with msm_precompute, exactly as a key load does
    for (int t = 0; t < N_TABLES; t++) {
      if (int rc = radix_convert(k->device, t == T_B2, buf + b.off_pts[t], k->h.npts[t], false)) return rc;
    }
    k->base_arena = std::move(buf);
    k->base_arena_len = b.total_len;
  }
  *dev_ptr = k->base_arena;
  *len = k->base_arena_len;
  return 0;
}

}  // extern "C"
namespace zkr {
// The full arena a compact one stands for, rebuilt on `device` into `arena_out`: sections copied to their
// places in THE layout, window levels and twiddles recomputed.  The receiver of a replica makes a key of it
// (zkr_key_adopt_base_arena); zkr_key_contribution_verify compares it with the arena it was handed.
int arena_from_base(const void *dev_ptr, size_t len, int device, Dev<unsigned char> &arena_out, ArenaHeader *h_out) {
  ZKR_HIP_CHECK(hipSetDevice(device));
  if (len < ARENA_HEADER_BYTES) { set_error("compact arena too small"); return ZKR_ERR_BAD_KEY; }
  ArenaHeader b;
  ZKR_HIP_CHECK(hipMemcpy(&b, dev_ptr, sizeof(b), hipMemcpyDeviceToHost));
  if (b.magic != BASE_MAGIC || b.total_len != len) { set_error("compact arena header mismatch (magic/len)"); return ZKR_ERR_BAD_KEY; }
  // the full layout, exactly as key_build lays it out
  ArenaHeader h = b;
  h.magic = ARENA_MAGIC;
  if (const char *fault = window_fault(h)) { set_error("compact arena: %s", fault); return ZKR_ERR_BAD_KEY; }
  MsmPlan plan[N_TABLES];
  for (int t = 0; t < N_TABLES; t++) plan[t] = msm_plan(rank_entries(h, t), h.npts[t], (int)h.win_c[t]);
  if (h.sc_n[0] > h.n || h.sc_lo[0] > h.n - h.sc_n[0] || h.sc_n[1] > h.m || h.sc_lo[1] > h.m - h.sc_n[1]) { set_error("compact arena: scalar ranges outside the vectors"); return ZKR_ERR_BAD_KEY; }
  arena_layout(h);
  const size_t off = h.total_len;
  // every section of the compact form lies inside the bytes handed over (a truncated or edited header must not drive the copies)
  {
    if (h.logm > 27 || h.m != (1u << h.logm) || h.n == 0 || h.p >= h.n) { set_error("compact arena: inconsistent sizes"); return ZKR_ERR_BAD_KEY; }
    auto inside = [&](uint64_t o, uint64_t bytes) { return o >= ARENA_HEADER_BYTES && o <= len && bytes <= len - o; };
    bool ok = true;
    for (int s = 0; s < 2 && ok; s++) {
      const uint64_t nnz = s == 0 ? h.nnzA : h.nnzB;
      ok = h.n_wide[s] <= h.m && inside(b.off_rowptr[s], ((uint64_t)h.m + 1) * 4) && inside(b.off_col[s], nnz * 4) && inside(b.off_coef[s], nnz * 32) &&
           inside(b.off_wide[s], (uint64_t)h.n_wide[s] * 4);
    }
    for (int t = 0; t < N_TABLES && ok; t++) {
      const uint64_t nsc = rank_entries(h, t);
      ok = h.npts[t] <= nsc && inside(b.off_pts[t], (uint64_t)h.npts[t] * (t == T_B2 ? 128 : 64)) && inside(b.off_rank[t], nsc * 4);
    }
    if (!ok) { set_error("compact arena: a section lies outside the %zu bytes handed over", len); return ZKR_ERR_BAD_KEY; }
  }
  Dev<unsigned char> arena;
  if (int arc = arena.alloc(off)) return arc;
  if (hipMemset(arena, 0, off) != hipSuccess) { set_error("hipMemset failed"); return ZKR_ERR_HIP; }  // as key_build: gaps and slack are defined bytes
  const unsigned char *src = (const unsigned char *)dev_ptr;
  auto cp = [&](uint64_t dst, uint64_t from, size_t bytes) { return bytes ? hipMemcpy(arena + dst, src + from, bytes, hipMemcpyDeviceToDevice) : hipSuccess; };
  hipError_t e = hipMemcpy(arena, &h, sizeof(h), hipMemcpyHostToDevice);
  for (int s = 0; s < 2 && e == hipSuccess; s++) {
    uint32_t nnz = s == 0 ? h.nnzA : h.nnzB;
    e = cp(h.off_rowptr[s], b.off_rowptr[s], ((size_t)h.m + 1) * 4);
    if (e == hipSuccess) e = cp(h.off_col[s], b.off_col[s], (size_t)nnz * 4);
    if (e == hipSuccess) e = cp(h.off_coef[s], b.off_coef[s], (size_t)nnz * 32);
    if (e == hipSuccess) e = cp(h.off_wide[s], b.off_wide[s], (size_t)h.n_wide[s] * 4);
  }
  for (int t = 0; t < N_TABLES && e == hipSuccess; t++) {
    e = cp(h.off_pts[t], b.off_pts[t], (size_t)h.npts[t] * (t == T_B2 ? 128 : 64));
    if (e == hipSuccess) e = cp(h.off_rank[t], b.off_rank[t], (size_t)rank_entries(h, t) * 4);
  }
  if (e != hipSuccess) { set_error("unpacking the compact arena failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  // the unpacked rows and rank maps before anything is built from them (the window levels and twiddles are rebuilt below)
  if (int crc = key_arena_check(device, arena, h, 0, nullptr)) return crc;
  for (int t = 0; t < N_TABLES; t++)
    if (int rc = msm_precompute(device, t == T_B2, arena + h.off_pts[t], h.npts[t], plan[t])) return rc;
  ntt_twiddles_fill((Fr *)(arena + h.off_tw), h.logm, (Fr *)(arena + h.off_twl), nullptr);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("rebuilding the window tables failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  arena_out = std::move(arena);
  *h_out = h;
  return 0;
}
}  // namespace zkr
extern "C" {

int zkr_key_adopt_base_arena(const void *dev_ptr, size_t len, int device, zkr_key **out) {
  if (!dev_ptr || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  Dev<unsigned char> arena;
  ArenaHeader h;
  if (int brc = arena_from_base(dev_ptr, len, device, arena, &h)) return brc;
  return key_from_arena(device, std::move(arena), h, out);
}

int zkr_key_save(const zkr_key *k, const char *path) {
  if (!k || !path) { set_error("null argument"); return ZKR_ERR_ARG; }
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  FILE *f = fopen(path, "wb");
  if (!f) { set_error("cannot open %s for writing", path); return ZKR_ERR_ARG; }
  const size_t CHUNK = (size_t)64 << 20;
  PinnedBuf stage;
  int rc = stage.alloc(CHUNK);
  for (size_t off = 0; !rc && off < k->arena_len; off += CHUNK) {
    size_t nb = k->arena_len - off < CHUNK ? k->arena_len - off : CHUNK;
    hipError_t e = hipMemcpy(stage, k->arena + off, nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_error("arena download failed: %s", hipGetErrorString(e)); rc = ZKR_ERR_HIP; }
    else if (fwrite(stage, 1, nb, f) != nb) { set_error("short write to %s", path); rc = ZKR_ERR_ARG; }
  }
  if (fclose(f) != 0 && !rc) { set_error("close failed on %s", path); rc = ZKR_ERR_ARG; }
  return rc;
}

int zkr_key_load_file(const char *path, int device, zkr_key **out) {
  if (!path || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  FILE *f = fopen(path, "rb");
  if (!f) { set_error("cannot open %s", path); return ZKR_ERR_BAD_KEY; }
  ArenaHeader h;
  if (fread(&h, 1, sizeof(h), f) != sizeof(h) || h.magic != ARENA_MAGIC || h.total_len < ARENA_HEADER_BYTES) {
    fclose(f);
    set_error("%s is not a packed zkr key (bad header)", path);
    return ZKR_ERR_BAD_KEY;
  }
  fseek(f, 0, SEEK_END);
  long flen = ftell(f);
  if (flen < 0 || (uint64_t)flen != h.total_len) { fclose(f); set_error("%s: length %ld != header total %llu", path, flen, (unsigned long long)h.total_len); return ZKR_ERR_BAD_KEY; }
  if (const char *fault = arena_header_fault(h, h.total_len)) { fclose(f); set_error("%s: %s", path, fault); return ZKR_ERR_BAD_KEY; }
  fseek(f, 0, SEEK_SET);
  Dev<unsigned char> arena;
  const size_t CHUNK = (size_t)64 << 20;
  PinnedBuf stage;
  hipError_t e;
  int rc = arena.alloc(h.total_len);
  if (!rc) rc = stage.alloc(CHUNK);
  for (size_t off = 0; !rc && off < h.total_len; off += CHUNK) {
    size_t nb = h.total_len - off < CHUNK ? h.total_len - off : CHUNK;
    if (fread(stage, 1, nb, f) != nb) { set_error("short read from %s", path); rc = ZKR_ERR_BAD_KEY; }
    else if ((e = hipMemcpy(arena + off, stage, nb, hipMemcpyHostToDevice)) != hipSuccess) { set_error("arena upload failed: %s", hipGetErrorString(e)); rc = ZKR_ERR_HIP; }
  }
  fclose(f);
  stage.reset();
  if (!rc) rc = key_arena_check(device, arena, h, 0, nullptr);
  if (rc) return rc;
  return key_from_arena(device, std::move(arena), h, out);
}

void zkr_free(void *p) { free(p); }

}  // extern "C"
