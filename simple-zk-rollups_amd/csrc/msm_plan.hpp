// msm_plan.hpp -- the host arithmetic that sizes one MSM (msm_plan) and says how the five tables of a key's proofs share digit
// sorts, bucket sets and reduction chains (proof_layout).  Nothing of HIP in it: the host shim compiles it for the CPU tests.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace zkr {

enum { T_A = 0, T_B1 = 1, T_B2 = 2, T_C = 3, T_H = 4, N_TABLES = 5 };

constexpr int MSM_THREADS = 256;
constexpr uint32_t MAX_RANGES = 256;  // x SORT_RANGE_MAX buckets = 2^21: window sizes up to c = 22 (2^24-point tables), or fused batches of small circuits
constexpr uint32_t SORT_RANGE_DEFAULT = 2048;   // buckets per range and records per (range, chunk) workgroup that msm_plan aims
constexpr uint32_t SORT_CHUNK_RECORDS = 3328;   // for (the L2 footprint of the scatter decides)
constexpr int LAT_GLOG = 3;  // reduction groups of a chain nothing can hide (a synchronous proof's last one): 2^3 buckets, see msm_reduce_enqueue
constexpr int ACC_ONTO = 1, ACC_ZERO_BIG = 2;  // flags of the accumulation kernels' `onto` argument

struct MsmPlan {
  int c, K, glog;
  uint32_t nbw, nb, big_thresh;  // nb = nbw = 2^(c-1) buckets, one set shared by the K windows
  uint32_t nR, nbl;   // digit sort: nR bucket ranges of nbl buckets (LDS counters of one workgroup)
  uint32_t J;         // digit sort: J chunks per bucket range
  uint32_t S;         // reduction: workgroups per task in msm_reduce2_kernel
};
// two tables whose bucket sets ONE reduction launch set can walk end to end (msm_reduce*_kernel take `batch` sets of one geometry)
inline bool same_reduce_geometry(const MsmPlan &a, const MsmPlan &b) { return a.c == b.c && a.K == b.K && a.nbw == b.nbw && a.nb == b.nb && a.glog == b.glog && a.S == b.S; }

// Oversized buckets (summed by msm_big_kernel's workgroups instead of one thread of the accumulation).  A bucket of E entries is
// E dependent additions on one lane -- 7 us each for G1, 18 us for G2 -- so any bucket longer than the accumulation's bulk
// time stretches the whole kernel: the bulk is the launch's additions (n K per proof, nbat proofs in a fused launch) at ~100 k
// additions per chain step chip-wide, i.e. the threshold is n K nbat / 2^17, between twice and eight times the mean occupancy,
// never below 64.  Round 3's rule (max(8 mean, 256)) left buckets of up to 256 entries to single lanes of SPARSE bucket sets: a
// shard of a 2^22 key (mean 9) spent 4.9 ms in a G2 accumulation of 0.8 ms of work (profiles/r4_25_shard_big_threshold.txt).
inline uint32_t big_threshold(size_t n, int K, uint32_t nbw, int nbat) {
  const uint64_t mean = (uint64_t)n * K / nbw + 1;
  const uint64_t by_bulk = ((uint64_t)n * K * (uint64_t)(nbat < 1 ? 1 : nbat)) >> 17;
  uint64_t thr = by_bulk < mean * 8 ? by_bulk : mean * 8;
  if (thr < 2 * mean) thr = 2 * mean;  // dense little bucket sets (tiny circuits): only real outliers leave the accumulation
  return thr > 64 ? (uint32_t)thr : 64u;
}

// Window size from the length of the SCALAR vector (tables that share scalars share the digit codes,
// kernels_msm.hpp msm_digits_kernel) unless the key fixes it (c_fixed: the window tables in the arena were built
// for that c); chunking and the oversized-bucket threshold from the table itself.
inline MsmPlan msm_plan(size_t n_scalars, size_t n, int c_fixed = 0) {
  MsmPlan pl;
  int lg = 0;
  while (((size_t)1 << lg) < n_scalars) lg++;
  int c = lg;  // 2^(c-1) buckets for ~n * 255/c entries: a few dozen entries per bucket
  if (c < 4) c = 4;
  // c stays at 20 above 2^20 scalars.  The digit sort takes up to 2^21 buckets (MAX_RANGES x SORT_RANGE_MAX), and by
  // multiplication counts c = 22 would pay at 2^24 points (12 instead of 13 additions per point for four times the
  // buckets: 1961 vs 2078 M multiplications per G1 table), but measured on the 2^24 rollup-shaped key it loses: 8.19 /
  // 7.50 proofs/s at c = 20 / 21, and at c = 22 the accumulation of a table takes 26.6 ms instead of 18 ms alone
  // (2 M bucket threads with short chains gather worse) and 3.5 -> 0.37 proofs/s with two proofs in flight; at 2^22
  // the counts already tie (530 / 544 / 532 M).  ZKR_MSM_C overrides (a documented knob: window bits of keys built in this process).
  if (c > 20) c = 20;
  if (const char *e = getenv("ZKR_MSM_C")) { int v = atoi(e); if (v >= 2 && v <= 22) c = v; }
  if (c_fixed) c = c_fixed;
  pl.c = c;
  pl.K = (255 + c - 1) / c;
  pl.nbw = 1u << (c - 1);
  pl.nb = pl.nbw;
  // bucket reduction in groups of 2^glog buckets (kernels_msm.hpp msm_reduce1_kernel: a chain of 2 * 2^glog - 2 additions
  // per thread).  At 2^19 buckets groups of 32 measured best (108 / 110 / 113 / 105 proofs/s at 8 / 16 / 32 / 64); with
  // fewer buckets the chip is not filled and the chain length is what counts: keep about 2^14 groups
  // (tx circuit, 2^16 buckets: 233 / 320 / 349 / 351 / 322 proofs/s at 32 / 16 / 8 / 4 / 2)
  int glog = c - 1 - 14 < 2 ? 2 : c - 1 - 14 > 5 ? 5 : c - 1 - 14;
  pl.glog = c - 1 < glog ? c - 1 : glog;
  pl.big_thresh = big_threshold(n, pl.K, pl.nbw, 1);
  // digit sort: one workgroup per (bucket range, chunk).  Ranges of 2048 buckets, chunks of ~3300 records: what counts is the
  // window of the entry array that the workgroups resident on one XCD scatter into together -- it has to stay in that XCD's
  // 4 MB L2 until its lines are complete (kernels_msm.hpp sort_block_to_chunk).  At 2^20 points: 256 ranges x 16 chunks, a
  // range's window is 212 KB, ~12 ranges in flight per XCD; with ranges of 8192 buckets (round 2) the same 16 chunks per range
  // kept 6.8 MB in flight per XCD and every line left L2 in pieces (WRITE_SIZE 386 MB per launch for 54 MB of entries, against
  // 98 MB now; kernel 159 -> 83 us; profiles/r3_ab_sort_ranges.md).
  uint32_t range_max = SORT_RANGE_DEFAULT;
  if (pl.nbw / range_max > MAX_RANGES) range_max = pl.nbw / MAX_RANGES;
  pl.nbl = pl.nbw < range_max ? pl.nbw : range_max;
  pl.nR = pl.nbw / pl.nbl;
  uint64_t J64 = ((uint64_t)n * pl.K + (uint64_t)pl.nR * SORT_CHUNK_RECORDS - 1) / ((uint64_t)pl.nR * SORT_CHUNK_RECORDS);
  uint32_t J = J64 > 64 ? 64u : (uint32_t)J64;
  if (J < 1) J = 1;
  pl.J = J;
  // reduction: every task sums ng/2 .. ng group results; one workgroup per 2048 of them, all tasks together at
  // most one workgroup per CU (msm_reduce3_kernel takes ntask * S <= MSM_THREADS partial sums)
  uint32_t ng = pl.nbw >> pl.glog, ntask = (uint32_t)(c - 1 - pl.glog) + 2;
  uint32_t S = (ng + 2047) / 2048;
  if (S > 16) S = 16;
  if (S > MSM_THREADS / ntask) S = MSM_THREADS / ntask;
  pl.S = S < 1 ? 1 : S;
  return pl;
}

// One reduction chain of a proof: the bucket sets of its member tables, end to end, walked by ONE reduction launch set.
struct ChainLayout {
  int n_members = 0;
  int members[2] = {-1, -1};  // tables in accumulation order
  int sets = 0;               // bucket sets (with their reduction buffers) per proof
  int geom = -1;              // the table whose plan sizes the sets and gives the reduction its geometry
  bool g2 = false;            // G2 points: reduced on the G2 chain's stream; G1 chains share the other
  bool latency = false;       // the proof's last chain: takes the latency-mode groups when the proof is alone (msm_reduce_enqueue)
};

// How the five tables of a key's proofs share digit sorts, bucket sets and reduction chains.  It depends on the key alone: worked
// out once from the point counts and the plans and read by every proof (zkr_prove.hip).  An empty table is in no chain.
struct ProofLayout {
  bool share_b = false, share_ac = false;  // B2 accumulates over B1's sort (same signals), C over A's (one support)
  int sort_src[N_TABLES] = {T_A, T_B1, T_B2, T_C, T_H};  // the table whose sort each table's accumulation reads
  int chain[N_TABLES] = {-1, -1, -1, -1, -1};  // the chain each table's sums land in
  int set[N_TABLES] = {0, 0, 0, 0, 0};         // ... and the bucket set within it
  int flags[N_TABLES] = {0, 0, 0, 0, 0};       // of its accumulation: ACC_ZERO_BIG / ACC_ONTO for the first / a later table of a SHARED set
  int n_chains = 0;
  ChainLayout chains[N_TABLES];  // in schedule order
  bool last_of_chain(int t) const { const ChainLayout &c = chains[chain[t]]; return c.members[c.n_members - 1] == t; }
  bool own_result(int t) const { return chain[t] >= 0 && flags[t] != ACC_ONTO; }  // else: empty, or summed into the result of the table it landed onto
};

// share_b / share_ac: what the key's header says about the tables' supports
inline ProofLayout proof_layout(const uint32_t npts[N_TABLES], bool share_b, bool share_ac, const MsmPlan plan[N_TABLES]) {
  ProofLayout L;
  L.share_b = share_b && npts[T_B1] == npts[T_B2];
  L.share_ac = share_ac && npts[T_A] == npts[T_C];  // A and C laid out over one support
  L.sort_src[T_B2] = L.share_b ? T_B1 : T_B2;
  L.sort_src[T_C] = L.share_ac ? T_A : T_C;
  auto open = [&](int t) -> ChainLayout & {
    ChainLayout &c = L.chains[L.n_chains];
    c.geom = t;
    c.g2 = t == T_B2;
    return c;
  };
  auto land = [&](ChainLayout &c, int t, int set, int flags) {
    c.members[c.n_members++] = t;
    c.sets = set + 1;
    L.chain[t] = (int)(&c - L.chains);
    L.set[t] = set;
    L.flags[t] = flags;
  };
  // B2 is alone: the only G2 table, first in the schedule (its chain is the longest)
  if (npts[T_B2]) { land(open(T_B2), T_B2, 0, 0); L.n_chains++; }
  // A and B1 in ONE reduction chain (round 5): the G1 chains share one stream, and in a single proof of a small circuit that stream
  // is the critical path from B1's accumulation to the end (three chains of ~0.4 ms back to back: H's chain starts 0.19 ms after H's
  // accumulation has ended, profiles/r4_05_timeline_one_tx_proof.txt).  A is accumulated into the bucket sets BEHIND B1's (the
  // chain holds two sets per proof when the two tables' geometry agrees) and one launch set reduces both: a chain of
  // latency-bound launches less per proof.
  const bool joint_ab = npts[T_A] && npts[T_B1] && same_reduce_geometry(plan[T_A], plan[T_B1]);
  if (npts[T_B1]) {
    ChainLayout &c = open(T_B1);
    land(c, T_B1, 0, 0);
    if (joint_ab) land(c, T_A, 1, 0);
    L.n_chains++;
  }
  if (npts[T_A] && !joint_ab) { land(open(T_A), T_A, 0, 0); L.n_chains++; }
  // C and H are only ever needed as C + H (App. B step 4: pi_c): when their bucket geometry agrees, H is accumulated ONTO
  // C's bucket set and one reduction chain serves both -- a bucket reduction (2 x 2^19 full additions, ~1.6 % of a proof's
  // instructions) and one latency chain less.  Oversized buckets of either table are ADDED to the shared set after H's
  // accumulation (C's accumulation clears their slots), so no accumulation waits for a reduction stream.
  const MsmPlan &pc = plan[T_C], &ph = plan[T_H];
  const bool merge_ch = npts[T_C] && npts[T_H] && pc.c == ph.c && pc.nbw == ph.nbw && pc.glog == ph.glog && pc.S == ph.S;
  if (npts[T_C]) {
    ChainLayout &c = open(merge_ch ? T_H : T_C);
    land(c, T_C, 0, merge_ch ? ACC_ZERO_BIG : 0);
    if (merge_ch) { land(c, T_H, 0, ACC_ONTO); c.latency = true; }
    L.n_chains++;
  }
  if (npts[T_H] && !merge_ch) { ChainLayout &c = open(T_H); land(c, T_H, 0, 0); c.latency = true; L.n_chains++; }
  return L;
}

}  // namespace zkr
