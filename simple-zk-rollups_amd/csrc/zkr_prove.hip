// zkr_prove.hip -- the hot path: one Groth16 proof on one MI355X.
//
// Replaces `await wasmBn128.groth16GenProof(witnessBin, provingKeyBin)`
// (/root/reference/operator/src/snarks/common.ts:29, scripts/index.js:46).  Stages:
//   ingest -> QAP rows (SpMV) -> 6 NTTs of size m (h = upper half of A.B) -> 5 MSMs -> host assembly.
// Everything up to the result point of each MSM runs on the GPU with no host round trip (streams and the
// two-proof pipeline: prove_submit below); the host then does the blinding arithmetic of App. B step 4
// (six 254-bit scalar multiplications) and the affine conversion.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <memory>
#include "eval_h.hpp"  // fr_root_of_unity
#include "kernels_msm.hpp"
#include "kernels_ntt.hpp"
#include "zkr_internal.hpp"

namespace zkr {

// ------------------------------------------------------------------ profiling (hipEvents on the launch stream)
static const char *STAGES[] = {"ingest", "spmv", "ntt", "msm_sort", "msm_accum_g1", "msm_accum_g2", "msm_big", "msm_reduce", "total",
                               "spmv_a", "ntt_pass", "combine_h"};  // the streaming kernels one by one (bench.py roofline.streaming): one QAP side, one NTT pass, the h combination
static int stage_index(const char *name) {
  for (int i = 0; i < (int)(sizeof(STAGES) / sizeof(STAGES[0])); i++)
    if (!strcmp(STAGES[i], name)) return i;
  return -1;
}
static hipEvent_t next_event(ProofSlot &sl) {  // nullptr when the runtime cannot create another event
  if (sl.event_next == sl.event_pool.size()) {
    ScopedEvent e;
    if (e.create()) return nullptr;
    sl.event_pool.push_back(std::move(e));
  }
  return sl.event_pool[sl.event_next++];
}
int prof_begin(Prof pf, hipStream_t s, const char *stage) {
  if (!pf.k || !pf.sl || !pf.k->prof_on) return -1;
  ProfSpan sp;
  sp.stage = stage_index(stage);
  sp.e0 = next_event(*pf.sl);
  sp.e1 = sp.e0 ? next_event(*pf.sl) : nullptr;
  if (!sp.e0 || !sp.e1) return -1;  // no timing for this span; the launch itself is unaffected
  hipEventRecord(sp.e0, s);
  pf.sl->spans.push_back(sp);
  return (int)pf.sl->spans.size() - 1;
}
void prof_end(Prof pf, hipStream_t s, int span) {
  if (span < 0) return;
  hipEventRecord(pf.sl->spans[span].e1, s);
}
int prof_collect(zkr_key *k, ProofSlot &sl) {  // call after the slot's work has completed
  if (k->stages.empty())
    for (auto nm : STAGES) { ProfStage st; st.name = nm; k->stages.push_back(st); }
  for (auto &sp : sl.spans) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, sp.e0, sp.e1) == hipSuccess && sp.stage >= 0) {
      k->stages[sp.stage].ms += ms;
      k->stages[sp.stage].launches++;
    }
  }
  sl.spans.clear();
  sl.event_next = 0;
  return 0;
}

// ------------------------------------------------------------------ NTT driver
struct PassSpec { int lo, hi, wlog; };
// tile_log: log2 of the elements a workgroup keeps in LDS (NTT_TILE_LOG, or less for small transforms: ntt_tile_log)
static std::vector<PassSpec> ntt_plan(int L, int tile_log) {
  // contiguous pass: low min(L, tile_log) stages; the rest in balanced chunks of <= 9 stages, listed top-down
  std::vector<PassSpec> v;
  int lows = L < tile_log ? L : tile_log;
  int rem = L - lows;
  if (rem > 0) {
    const int strided = NTT_STRIDED_LOG < tile_log - 1 ? NTT_STRIDED_LOG : tile_log - 1;  // at least two columns (64 contiguous bytes) per row
    int nch = (rem + strided - 1) / strided;
    int hi = L;
    for (int i = 0; i < nch; i++) {
      int nb = (rem + (nch - i) - 1) / (nch - i);
      int lo = hi - nb;
      int wlog = tile_log - nb;
      if (wlog > lo) wlog = lo;
      v.push_back({lo, hi, wlog});
      hi = lo;
      rem -= nb;
    }
  }
  v.push_back({0, lows, 0});
  return v;
}

// the butterflies' twiddle tables (x 2^261, one entry more than the x 2^256 tables they are made from; kernels_ntt.hpp)
int ntt_tables29_build(const Fr *tw, uint32_t n_tw, const Fr *twl, uint32_t n_twl, hipStream_t s, Dev<Tw29> &tw29, Dev<Tw29> &twl29) {
  Dev<Tw29> a, b;
  int rc;
  if ((rc = a.alloc((size_t)n_tw + 1)) || (rc = b.alloc((size_t)n_twl + 1))) return rc;
  twiddle261_kernel<<<(n_tw + 256) / 256, 256, 0, s>>>(tw, n_tw, a);
  twiddle261_kernel<<<(n_twl + 256) / 256, 256, 0, s>>>(twl, n_twl, b);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipStreamSynchronize(s));  // the proving streams are non-blocking: they do not order themselves after this one
  tw29 = std::move(a);
  twl29 = std::move(b);
  return 0;
}
// the x 2^256 tables those are made from: tw[i] = w_{2^(k+1)}^i for i < 2^k, and the local table twl[i] = w_2048^i for i < 2^TWL_LOG
void ntt_twiddles_fill(Fr *tw, unsigned k, Fr *twl, hipStream_t s) {
  const uint32_t n = 1u << k, nl = 1u << TWL_LOG;
  twiddle_table_kernel<<<(n + 255) / 256, 256, 0, s>>>(tw, n, fr_root_of_unity(k + 1));
  twiddle_table_kernel<<<(nl + 255) / 256, 256, 0, s>>>(twl, nl, fr_root_of_unity(TWL_LOG + 1));
}
// The tables of a stage hook (zkr_ntt, zkr_selftest_ntt), which has no key to take them from: built for 2^tlog on the null stream
struct HookNttTables {
  DevBuf tw, twl;
  Dev<Tw29> tw29, twl29;
  int tlog = 0;
  int build(unsigned log) {
    tlog = (int)log;
    int rc;
    if ((rc = tw.alloc((size_t)32 << log)) || (rc = twl.alloc((size_t)32 << TWL_LOG))) return rc;
    ntt_twiddles_fill(tw.as<Fr>(), log, twl.as<Fr>(), nullptr);
    return ntt_tables29_build(tw.as<Fr>(), 1u << log, twl.as<Fr>(), 1u << TWL_LOG, nullptr, tw29, twl29);
  }
  NttTables view() const { return NttTables{tw.as<Fr>(), tw29, twl29, tlog}; }
};

// An NTT pass keeps a tile of 2^NTT_TILE_LOG elements x 9 limbs in LDS: 72 KB, above the 64 KB every target before gfx950
// offers.  Asked once per device, so that another architecture (the Makefile's ARCH can be overridden) fails at key load / in
// zkr_ntt with this message instead of a generic launch error deep inside a proof.
int ntt_lds_check(int device) {
  int lds = 0;
  ZKR_HIP_CHECK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  const int need = 36 << NTT_TILE_LOG;
  if (lds < need) {
    set_error("device %d offers %d bytes of LDS per workgroup, the NTT passes need %d (built for gfx950: 160 KB per CU)", device, lds, need);
    return ZKR_ERR_NO_DEVICE;
  }
  return 0;
}

// Elements per workgroup: 2048 (NTT_TILE_LOG) for every transform.  Smaller tiles for small transforms -- a 2^17 transform cut into
// tiles of 2048 is 64 workgroups, a quarter of the CUs -- were measured (512 / 1024 elements) and change nothing: the wavefront
// count of a transform does not depend on the tile (a single tx proof 2.00 / 2.04 / 1.97-2.02 ms, profiles/r4_19_tx_single_ntt_tile.txt).

// A transform call says what it passes by name.  The butterfly and the sign of the exponent are ONE choice out of four:
enum NttDir { DIF_INVERSE, DIF_FORWARD, DIT_FORWARD, DIT_INVERSE };  // DIF: natural in, bit-reversed out; DIT: the other way round
struct NttVecs { const Fr *in0 = nullptr, *in1 = nullptr; Fr *out = nullptr; };  // one transform's vectors; in1 with PRE_MUL only: the transform of in0 . in1
static NttVecs ntt_in_place(Fr *v) { return NttVecs{v, nullptr, v}; }
// One transform, or TWO of the same shape in the same launches (b: gridDim.z = 2)
// want_lo / want_n (DIF only; 0, 0 = everything): only positions [want_lo, want_lo + want_n) of the output are wanted -- the
// passes run on the aligned blocks that cover them (kernels_ntt.hpp NttPassArgs::blk_off); the rest of `out` is left half done
struct NttRun {
  int L;
  NttDir dir;
  int pre = PRE_NONE, nbat = 1;  // nbat vectors end to end in every buffer
  NttVecs a, b;                  // b.out null: one transform
  uint32_t want_lo = 0, want_n = 0;
  uint32_t coset_shift = 0, coset_add = 0;  // PRE_COSET when the transform is one block of a larger one (NttPassArgs::pre_shift; calc_h_split)
};

// what every pass of either driver is told
static NttPassArgs ntt_pass_args(const NttTables &tb, int L) {
  NttPassArgs a = {};
  a.tw = tb.tw; a.tw29 = tb.tw29; a.twl29 = tb.twl29; a.tlog = tb.tlog; a.L = L;
  // wave priority 1 for the NTT passes: with the 29-bit-limb accumulations the preparation chain (sorts + calcH) became
  // the stream that paces two proofs in flight (its kernels starved behind the accumulation's wavefronts: 4.1 ms of NTT
  // spans per proof at priority 0, 2.9 ms at 1; 120.9 -> 125.2 proofs/s; 2 and 3 measure the same as 1)
  a.prio = 1;
  return a;
}
template <int T, bool CROSS>
static void ntt_pass_launch_dir(NttDir dir, dim3 grid, size_t lds, hipStream_t s, const NttPassArgs &a) {
  switch (dir) {
    case DIF_INVERSE: ntt_pass_kernel<true, true, T, CROSS><<<grid, T, lds, s>>>(a); break;
    case DIF_FORWARD: ntt_pass_kernel<true, false, T, CROSS><<<grid, T, lds, s>>>(a); break;
    case DIT_FORWARD: ntt_pass_kernel<false, false, T, CROSS><<<grid, T, lds, s>>>(a); break;
    case DIT_INVERSE: ntt_pass_kernel<false, true, T, CROSS><<<grid, T, lds, s>>>(a); break;  // only zkr_selftest_ntt asks for it
  }
}
// One pass inside its `ntt_pass` span: THE place that names the kernel's instantiations -- the four directions at either
// workgroup size, and as CROSS passes at NTT_THREADS_LARGE only (whatever `threads` says)
static void ntt_pass_launch(int threads, bool cross, NttDir dir, dim3 grid, size_t lds, hipStream_t s, const NttPassArgs &a, Prof pf) {
  const int psp = prof_begin(pf, s, "ntt_pass");
  if (cross) ntt_pass_launch_dir<NTT_THREADS_LARGE, true>(dir, grid, lds, s, a);
  else if (threads == NTT_THREADS_SMALL) ntt_pass_launch_dir<NTT_THREADS_SMALL, false>(dir, grid, lds, s, a);
  else ntt_pass_launch_dir<NTT_THREADS_LARGE, false>(dir, grid, lds, s, a);
  prof_end(pf, s, psp);
}

static int run_ntt(hipStream_t s, const NttTables &tb, const NttRun &r, Prof pf) {
  const int L = r.L;
  const bool dif = r.dir == DIF_INVERSE || r.dir == DIF_FORWARD;
  if (r.want_n && (!dif || (uint64_t)r.want_lo + r.want_n > (1ull << L))) { set_error("run_ntt: an output range needs a DIF transform and must lie inside it"); return ZKR_ERR_ARG; }
  std::vector<PassSpec> plan = ntt_plan(L, NTT_TILE_LOG);
  if (!dif) std::reverse(plan.begin(), plan.end());
  bool first = true;
  for (auto &ps : plan) {
    NttPassArgs a = ntt_pass_args(tb, L);
    a.pre_shift = r.coset_shift; a.pre_add = r.coset_add;
    a.in0 = first ? r.a.in0 : r.a.out;
    a.in1 = first ? r.a.in1 : nullptr;
    a.out = r.a.out;
    a.in0_b = first ? r.b.in0 : r.b.out;
    a.in1_b = first ? r.b.in1 : nullptr;
    a.out_b = r.b.out;
    a.lo = ps.lo; a.hi = ps.hi; a.wlog = ps.wlog;
    a.pre = first ? r.pre : PRE_NONE;
    a.canon = &ps == &plan.back() ? 1 : 0;  // between passes values stay lazily reduced (below 3 r)
    uint32_t tile = 1u << (ps.hi - ps.lo + ps.wlog);
    uint32_t grid = (1u << L) / tile;
    a.blk_off = 0;
    if (r.want_n) {  // the 2^hi-blocks that cover the range, 2^hi / tile workgroups each
      const uint32_t per_block = (1u << ps.hi) / tile;
      const uint32_t q0 = r.want_lo >> ps.hi, q1 = (uint32_t)(((uint64_t)r.want_lo + r.want_n + (1u << ps.hi) - 1) >> ps.hi);
      a.blk_off = q0 * per_block;
      grid = (q1 - q0) * per_block;
    }
    size_t lds = (size_t)tile * 36;  // 9 limbs per element
    // workgroup size by transform size (kernels_ntt.hpp NTT_THREADS_*); a tile of 1024 elements has 256 four-element butterfly
    // groups per double stage: 256 threads
    const int threads = (L >= NTT_LARGE_LOG || tile <= 1024) ? NTT_THREADS_LARGE : NTT_THREADS_SMALL;
    ntt_pass_launch(threads, false, r.dir, dim3(grid, r.nbat, r.b.out ? 2 : 1), lds, s, a, pf);
    first = false;
  }
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

static Fr fr_from_u64(uint64_t x) {
  Fr r = Fr::zero();
  r.v[0] = (uint32_t)x;
  r.v[1] = (uint32_t)(x >> 32);
  return r;
}

// QAP rows [lo, hi) of nbat witnesses end to end (sl.d_w -> sl.va, sl.vb): both sides in one launch (blockIdx.z; one launch fewer in
// the chain, twice the workgroups), then the rows wider than SPMV_WIDE terms
// with_c (H in evaluation form): the C side too -- witness j's row sums into sl.d_h + j m, free until the coset products land there --
// and the slot's nbat counters of unsatisfied rows cleared for the check that follows
static void spmv_enqueue(zkr_key *k, ProofSlot &sl, hipStream_t s, uint32_t lo, uint32_t hi, int nbat, bool with_c = false) {
  const Prof pf{k, &sl};
  const ArenaHeader &h = k->h;
  const unsigned char *ar = k->arena;
  const int sp = prof_begin(pf, s, "spmv");
  SpmvSide side[3] = {};
  Fr *evals[2] = {sl.va, sl.vb};
  for (int i = 0; i < 2; i++)
    side[i] = SpmvSide{(const uint32_t *)(ar + h.off_rowptr[i]), (const uint32_t *)(ar + h.off_col[i]), (const Fr *)(ar + h.off_coef[i]), evals[i],
                       (const uint32_t *)(ar + h.off_wide[i]), h.n_wide[i]};
  const EvalTables &ev = k->eval;
  if (with_c) side[2] = SpmvSide{ev.c_rowptr, ev.c_col, ev.c_coef, sl.d_h, ev.c_wide, ev.n_wide};
  const unsigned sides = with_c ? 3 : 2;
  const int sa = prof_begin(pf, s, "spmv_a");
  spmv_kernel<<<dim3((hi - lo + 255) / 256, nbat, sides), 256, 0, s>>>(side[0], side[1], side[2], sl.d_w, h.m, h.n, lo, hi, with_c ? sl.d_bad : nullptr);
  prof_end(pf, s, sa);
  uint32_t nw = h.n_wide[0] > h.n_wide[1] ? h.n_wide[0] : h.n_wide[1];
  if (with_c && ev.n_wide > nw) nw = ev.n_wide;
  if (nw) spmv_wide_kernel<<<dim3(nw, nbat, sides), 64, 0, s>>>(side[0], side[1], side[2], sl.d_w, h.m, h.n, lo, hi);
  prof_end(pf, s, sp);
}

// constants of the combination: S' = m S / R, D' = m^3 D g^i / R  ->  h = S'*R^2/(2m) (*1/R)  -  D' g^-i * R^2/(2 m^3) (*1/R)
static void combine_h_consts(uint32_t m, Fr &c1v, Fr &c2v) {
  Fr r2 = Fr::r2();
  Fr minv = inv(to_mont(fr_from_u64(m)));        // Montgomery(1/m)
  Fr half = inv(to_mont(fr_from_u64(2)));        // Montgomery(1/2)
  c1v = mul(mul(r2, half), minv);                // value R^2/(2m) ... as plain integer: from_mont of Montgomery product chain
  // r2 is the integer R^2 mod r = Montgomery(R).  mul(r2, half) = Montgomery(R/2); times minv = Montgomery(R/(2m)).
  // We need the plain integer R^2/(2m) = Montgomery(R/(2m)) exactly, so c1v is already the constant to pass.
  c2v = mul(mul(c1v, minv), minv);               // Montgomery(R/(2m^3)) = integer R^2/(2m^3)
}

static NttTables key_ntt_tables(const zkr_key *k) { return NttTables{(const Fr *)(k->arena + k->h.off_tw), k->tw29, k->twl29, (int)k->h.tlog}; }

// What the two replicated forms do first after their QAP rows, nbat witnesses end to end: the `ntt` span opens (the caller closes
// it), then two pairs of transforms of the same shape, each pair in ONE set of launches (gridDim.z = 2): the coefficients of a and
// b (sl.va, sl.vb -> sl.ca, sl.cb; x m, bit-reversed), then their evaluations on the coset g*w^c in place (x m, natural)
static int calc_h_open(zkr_key *k, ProofSlot &sl, hipStream_t s, int nbat, int *ntt_span) {
  const Prof pf{k, &sl};
  const NttTables tb = key_ntt_tables(k);
  const int L = (int)k->h.logm;
  *ntt_span = prof_begin(pf, s, "ntt");
  if (int rc = run_ntt(s, tb, NttRun{.L = L, .dir = DIF_INVERSE, .nbat = nbat, .a = {.in0 = sl.va, .out = sl.ca}, .b = {.in0 = sl.vb, .out = sl.cb}}, pf)) return rc;
  return run_ntt(s, tb, NttRun{.L = L, .dir = DIT_FORWARD, .pre = PRE_COSET, .nbat = nbat, .a = ntt_in_place(sl.ca), .b = ntt_in_place(sl.cb)}, pf);
}

// d_w (std, reduced) -> d_h (std, bit-reversed order), nbat vectors end to end.  See DESIGN.md "calcH on the GPU".
static int calc_h_device(zkr_key *k, ProofSlot &sl, hipStream_t s, int nbat) {
  const Prof pf{k, &sl};
  const ArenaHeader &h = k->h;
  const NttTables tb = key_ntt_tables(k);
  const int L = (int)h.logm;
  uint32_t m = h.m;
  spmv_enqueue(k, sl, s, 0, m, nbat);
  int sp, rc;
  // The six transforms come in three pairs of the same shape: the two of calc_h_open, then the pair of inverse transforms below.
  // A shard multiplies only positions [sc_lo, sc_lo + sc_n) of h (bit-reversed order, as the H table is laid out): the last pair of
  // transforms -- inverse DIF, whose passes below the top one stay inside aligned blocks -- and the combination run on the
  // blocks that cover that range only (at 2^22: 16 of 22 stages of two of the six transforms on 1/8 of the vector for 8 shards).
  const bool ranged = h.shard_parts > 1 && h.sc_n[1] < m;
  const uint32_t h_lo = ranged ? h.sc_lo[1] : 0, h_n = ranged ? h.sc_n[1] : 0;
  if ((rc = calc_h_open(k, sl, s, nbat, &sp))) return rc;
  // then D' = iNTT(A(gw^c).B(gw^c)) and S' = iNTT(a.b), both unscaled and bit-reversed
  if ((rc = run_ntt(s, tb, NttRun{.L = L, .dir = DIF_INVERSE, .pre = PRE_MUL, .nbat = nbat, .a = {.in0 = sl.ca, .in1 = sl.cb, .out = sl.ca},
                                  .b = {.in0 = sl.va, .in1 = sl.vb, .out = sl.va}, .want_lo = h_lo, .want_n = h_n}, pf))) return rc;
  Fr c1v, c2v;
  combine_h_consts(m, c1v, c2v);
  const int csp = prof_begin(pf, s, "combine_h");
  const uint32_t pos0 = ranged ? h_lo : 0, pos1 = ranged ? h_lo + h_n : m;
  combine_h_kernel<<<dim3((pos1 - pos0 + 255) / 256, nbat), 256, 0, s>>>(sl.va, sl.ca, sl.d_h, tb.tw, tb.tlog, L, c1v, c2v, sl.dig_h.rng, DIGIT_CLEAR_WORDS, pos0, pos1);  // + the counters of h's digit records
  prof_end(pf, s, csp);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// H in evaluation form (a key with side tables, EvalTables; eval_h.hpp): d_w -> the coset products d_j in sl.d_h, natural order.
// Four transforms instead of six and no combination: QAP rows of A, B and C in one launch, the count of rows with a_j b_j != c_j
// into the slot's pinned words (prove_collect reads them with the proofs' results), the two coefficient transforms, the two coset
// transforms (canonical stores on their last pass), one product per row.  nbat witnesses end to end (a fused group) share every
// launch: vectors at stride m, one counter word per witness, ONE copy of the nbat words.
// A shard with side tables (zkr_key_shard_opts) in a sharded proof that computes h on every shard: the same sequence over the whole
// domain -- every shard counts all the rows -- but the product is made over the shard's range of d only, the scalars its part of E'
// takes (natural order: the range is contiguous).
static int calc_h_eval(zkr_key *k, ProofSlot &sl, hipStream_t s, int nbat) {
  const Prof pf{k, &sl};
  const ArenaHeader &h = k->h;
  const uint32_t m = h.m;
  spmv_enqueue(k, sl, s, 0, m, nbat, true);
  eval_unsatisfied_kernel<<<dim3((m + 255) / 256, nbat), 256, 0, s>>>(sl.va, sl.vb, sl.d_h, m, sl.d_bad, 0, m);
  ZKR_HIP_CHECK(hipMemcpyAsync(sl.h_bad, sl.d_bad, (size_t)nbat * 4, hipMemcpyDeviceToHost, s));
  const uint32_t d0 = h.sc_lo[1], d1 = h.sc_lo[1] + h.sc_n[1];  // a whole key: 0 and m
  int sp;
  if (int rc = calc_h_open(k, sl, s, nbat, &sp)) return rc;
  const int csp = prof_begin(pf, s, "combine_h");  // the stage record keeps its keys: the product stands where the combination stood
  eval_product_kernel<<<dim3((d1 - d0 + 255) / 256, nbat), 256, 0, s>>>(sl.ca, sl.cb, sl.d_h, m, sl.dig_h.rng, DIGIT_CLEAR_WORDS, d0, d1);
  prof_end(pf, s, csp);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ calcH split over the shards of one proof
thread_local ShardGroup *shard_group = nullptr;
thread_local unsigned shard_group_part = 0;
thread_local bool shard_turn_held = false;

// The top klog stages of a transform of 2^L points whose 2^klog blocks live in different buffers (kernels_ntt.hpp CROSS): this
// shard's columns [col_lo, col_lo + col_n) of every block.  rows_*[r]: where block r starts (x_sub = 0) or where this shard's
// columns of block r start in a local buffer (x_sub = col_lo).
// log2 of the columns per tile: a full tile's, or as many as the shard has (col_lo and col_n must be multiples of it)
static int ntt_cross_wlog(int klog, uint32_t col_n) {
  int wlog = NTT_TILE_LOG - klog;
  while ((1u << wlog) > col_n) wlog--;
  return wlog;
}
struct NttCross {
  int L, klog;
  NttDir dir;
  int pre = PRE_NONE;
  bool canon = false;  // the transform's last pass: canonical stores
  const Fr *const *rows_in0, *const *rows_in1 = nullptr;  // rows_in1 with PRE_MUL only
  Fr *const *rows_out;
  uint32_t in_sub = 0, out_sub = 0, col_lo, col_n;
};
static int run_ntt_cross(hipStream_t s, const NttTables &tb, const NttCross &c, Prof pf) {
  NttPassArgs a = ntt_pass_args(tb, c.L);
  a.lo = c.L - c.klog; a.hi = c.L;
  const int wlog = ntt_cross_wlog(c.klog, c.col_n);
  a.wlog = wlog;
  a.pre = c.pre;
  a.canon = c.canon ? 1 : 0;
  for (int r = 0; r < (1 << c.klog); r++) { a.x_in0[r] = c.rows_in0[r]; a.x_in1[r] = c.rows_in1 ? c.rows_in1[r] : nullptr; a.x_out[r] = c.rows_out[r]; }
  a.x_in_sub = c.in_sub; a.x_out_sub = c.out_sub;
  const uint32_t tile = 1u << (c.klog + wlog);
  a.blk_off = c.col_lo >> wlog;
  const uint32_t grid = c.col_n >> wlog;
  ntt_pass_launch(NTT_THREADS_LARGE, true, c.dir, dim3(grid), (size_t)tile * 36, s, a, pf);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// calcH of ONE proof split over the P = 2^klog shards that run it (zkr_prove_sharded): shard j owns block j -- positions
// [j m/P, (j + 1) m/P) -- of every vector, which is also its range of h.  Of a transform's log2 m stages all but the top klog stay
// inside a block; the top ones (first in the inverse DIF transforms, last in the forward DIT ones) pair the same column of
// different blocks, and run as CROSS passes in which shard j takes columns [j m/P^2, (j + 1) m/P^2) of every block, reading and
// writing the other shards' buffers directly (peer access; on one device: plain loads).  Per shard: 1/P of the QAP rows and 1/P
// of every transform's butterflies instead of four transforms in full and two in part.  Phases, with a host barrier of the
// group after each of the first four (every shard's stream is idle when its thread arrives):
//   1  QAP rows of the block                                                  -> va, vb (block j)
//   2  CROSS top stages of iNTT(a), iNTT(b), iNTT(a.b)   [all blocks' va, vb] -> ca, cb, d_h (this shard's columns of every block)
//   3  the blocks' own stages: rest of iNTT(a), iNTT(b); the coset transforms up to their top stages; rest of iNTT(a.b)
//   4  CROSS top stages of the coset transforms [all blocks' ca, cb] -> this shard's columns, kept locally (va, vb: free since 2);
//      their product; CROSS top stages of iNTT(product)                       -> ca (this shard's columns of every block)
//   5  the block's own stages of that; h = combination on the block           -> d_h (block j).  No barrier: the rest is the shard's own
// The enqueue lock of the device is released while the thread waits (shards on one device share its streams and its lock).
// eval -- H in evaluation form, every shard of the group with side tables (calc_h_eval has the sequence): the same five phases and
// four barriers with a third less in them.  The product of the coset evaluations is the end, so iNTT(a.b) and the last inverse
// transform go, and what block j must hold is d in NATURAL order:
//   1  QAP rows of the block for A, B and C (C's into the block of d_h, free until 5) and the count of its unsatisfied rows
//   2  CROSS top stages of iNTT(a), iNTT(b)              [all blocks' va, vb] -> ca, cb (this shard's columns of every block)
//   3  the blocks' own stages of the two; the coset transforms up to their top stages
//   4  CROSS top stages of the coset transforms, canonical, IN PLACE: this shard's columns of every block's ca, cb -- which no
//      other shard touches -- so that after the barrier block j of ca, cb on shard j holds the evaluations in natural order
//   5  d = their product on the block                                          -> d_h (block j)
static int calc_h_split(zkr_key *k, ProofSlot &sl, hipStream_t s, ShardGroup &g, unsigned part, std::unique_lock<std::mutex> &lock, bool eval) {
  struct AbortUnlessDone {  // on every return but the last: whoever waits for this shard (now or at a later barrier) gives up too
    ShardGroup &g;
    bool done = false;
    ~AbortUnlessDone() { if (!done) g.abort(); }
  } guard{g};
  const Prof pf{k, &sl};
  const ArenaHeader &h = k->h;
  const NttTables tb = key_ntt_tables(k);
  const int L = (int)h.logm, klog = g.klog, Lb = L - klog;
  const uint32_t m = h.m, P = g.parts, Bk = m >> klog, cols = Bk >> klog, col_lo = part * cols, blk = part * Bk;
  struct timespec t0;
  int phase = 0;
  auto phase_begin = [&] { clock_gettime(CLOCK_MONOTONIC, &t0); };
  auto phase_stamp = [&] {  // host time since the phase began, into the group's record
    struct timespec t1;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (phase < 8) g.phase_ms[part][phase] = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
  };
  // end of a phase: this shard's part of it has run, then everybody's
  auto phase_end = [&]() -> int {
    hipError_t e = hipGetLastError();
    lock.unlock();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    phase_stamp();
    phase++;
    int rc = 0;
    if (e != hipSuccess) { set_error("split calcH, phase %d: %s", phase, hipGetErrorString(e)); g.abort(); rc = ZKR_ERR_HIP; }
    else if (!g.barrier()) { set_error("split calcH: another shard of the proof failed"); rc = ZKR_ERR_HIP; }
    lock.lock();
    if (!rc) ZKR_HIP_CHECK(hipSetDevice(k->device));
    return rc;
  };
  int rc;
  // where this shard's vectors are: read by the others after the first barrier
  g.vecs[part] = ShardGroup::Vecs{sl.va, sl.vb, sl.ca, sl.cb, sl.d_h};
  if (g.solo)
    for (unsigned b = 0; b < P; b++) g.vecs[b] = g.vecs[part];
  // 1: QAP rows of the block
  phase_begin();
  spmv_enqueue(k, sl, s, blk, blk + Bk, 1, eval);
  if (eval) {  // the block's rows with a_j b_j != c_j; the count has landed when the phase ends (its stream is idle then)
    eval_unsatisfied_kernel<<<dim3((Bk + 255) / 256, 1), 256, 0, s>>>(sl.va, sl.vb, sl.d_h, m, sl.d_bad, blk, blk + Bk);
    ZKR_HIP_CHECK(hipMemcpyAsync(sl.h_bad, sl.d_bad, 4, hipMemcpyDeviceToHost, s));
  }
  if ((rc = phase_end())) return rc;
  const Fr *r_va[8], *r_vb[8], *r_ca[8], *r_cb[8], *r_ga[8], *r_gb[8];
  Fr *w_ca[8], *w_cb[8], *w_dh[8], *w_ga[8], *w_gb[8];
  for (unsigned b = 0; b < P; b++) {
    const ShardGroup::Vecs &v = g.vecs[b];
    r_va[b] = (const Fr *)v.va + (size_t)b * Bk; r_vb[b] = (const Fr *)v.vb + (size_t)b * Bk;
    r_ca[b] = w_ca[b] = (Fr *)v.ca + (size_t)b * Bk; r_cb[b] = w_cb[b] = (Fr *)v.cb + (size_t)b * Bk;
    w_dh[b] = (Fr *)v.dh + (size_t)b * Bk;
    r_ga[b] = w_ga[b] = sl.va + blk + (size_t)b * cols;  // this shard's columns of block b, kept in its own block of va / vb
    r_gb[b] = w_gb[b] = sl.vb + blk + (size_t)b * cols;
  }
  // the top klog stages of a transform of the whole domain, on this shard's columns of every block: the call names the rest
  auto top_stages = [&](NttCross c) { c.L = L; c.klog = klog; c.col_lo = col_lo; c.col_n = cols; return run_ntt_cross(s, tb, c, pf); };
  const int ntt_span = prof_begin(pf, s, "ntt");
  // 2: top stages of the three inverse transforms that start from the evaluations on the domain
  phase_begin();
  if ((rc = top_stages({.dir = DIF_INVERSE, .rows_in0 = r_va, .rows_out = w_ca}))) return rc;
  if ((rc = top_stages({.dir = DIF_INVERSE, .rows_in0 = r_vb, .rows_out = w_cb}))) return rc;
  if (!eval && (rc = top_stages({.dir = DIF_INVERSE, .pre = PRE_MUL, .rows_in0 = r_va, .rows_in1 = r_vb, .rows_out = w_dh}))) return rc;
  if ((rc = phase_end())) return rc;
  // 3: the block's own stages
  phase_begin();
  {
    Fr *ca = sl.ca + blk, *cb = sl.cb + blk, *dh = sl.d_h + blk;
    uint32_t rev = 0;  // the block's index bit-reversed: low bits of its coefficients' indices
    for (int i = 0; i < klog; i++) rev |= ((part >> i) & 1u) << (klog - 1 - i);
    // coefficients of a, b (x m, bit-reversed); coset transforms below their top stages; S' on the block
    if ((rc = run_ntt(s, tb, NttRun{.L = Lb, .dir = DIF_INVERSE, .a = ntt_in_place(ca), .b = ntt_in_place(cb)}, pf))) return rc;
    if ((rc = run_ntt(s, tb, NttRun{.L = Lb, .dir = DIT_FORWARD, .pre = PRE_COSET, .a = ntt_in_place(ca), .b = ntt_in_place(cb), .coset_shift = (uint32_t)klog, .coset_add = rev}, pf))) return rc;
    if (!eval && (rc = run_ntt(s, tb, NttRun{.L = Lb, .dir = DIF_INVERSE, .a = ntt_in_place(dh)}, pf))) return rc;
  }
  if ((rc = phase_end())) return rc;
  // 4: top stages of the coset transforms into local columns, product, top stages of the last inverse transform
  phase_begin();
  int csp;
  if (eval) {
    if ((rc = top_stages({.dir = DIT_FORWARD, .canon = true, .rows_in0 = r_ca, .rows_out = w_ca}))) return rc;
    if ((rc = top_stages({.dir = DIT_FORWARD, .canon = true, .rows_in0 = r_cb, .rows_out = w_cb}))) return rc;
    if ((rc = phase_end())) return rc;
    // 5: d on the block
    phase_begin();
    csp = prof_begin(pf, s, "combine_h");  // as in calc_h_eval: the product stands where the combination stood
    eval_product_kernel<<<dim3((Bk + 255) / 256, 1), 256, 0, s>>>(sl.ca, sl.cb, sl.d_h, m, sl.dig_h.rng, DIGIT_CLEAR_WORDS, blk, blk + Bk);
  } else {
    if ((rc = top_stages({.dir = DIT_FORWARD, .canon = true, .rows_in0 = r_ca, .rows_out = w_ga, .out_sub = col_lo}))) return rc;
    if ((rc = top_stages({.dir = DIT_FORWARD, .canon = true, .rows_in0 = r_cb, .rows_out = w_gb, .out_sub = col_lo}))) return rc;
    if ((rc = top_stages({.dir = DIF_INVERSE, .pre = PRE_MUL, .rows_in0 = r_ga, .rows_in1 = r_gb, .rows_out = w_ca, .in_sub = col_lo}))) return rc;
    if ((rc = phase_end())) return rc;
    // 5: D' on the block, then h
    phase_begin();
    if ((rc = run_ntt(s, tb, NttRun{.L = Lb, .dir = DIF_INVERSE, .a = ntt_in_place(sl.ca + blk)}, pf))) return rc;
    Fr c1v, c2v;
    combine_h_consts(m, c1v, c2v);
    csp = prof_begin(pf, s, "combine_h");
    combine_h_kernel<<<dim3((Bk + 255) / 256, 1), 256, 0, s>>>(sl.d_h, sl.ca, sl.d_h, tb.tw, tb.tlog, L, c1v, c2v, sl.dig_h.rng, DIGIT_CLEAR_WORDS, blk, blk + Bk);
  }
  prof_end(pf, s, csp);
  prof_end(pf, s, ntt_span);
  ZKR_HIP_CHECK(hipGetLastError());
  phase_stamp();  // enqueue time only: nothing waits here
  guard.done = true;
  return 0;
}

// ------------------------------------------------------------------ MSM driver
template <class F> struct MsmCfg;
template <> struct MsmCfg<Fq> { static constexpr int ACC_W = 2, SPLIT_W = 2; static constexpr bool ACC_AHEAD = true; static constexpr const char *ACC_STAGE = "msm_accum_g1"; };
template <> struct MsmCfg<Fq2> { static constexpr int ACC_W = 2, SPLIT_W = 1; static constexpr bool ACC_AHEAD = false; static constexpr const char *ACC_STAGE = "msm_accum_g2"; };  // a second 128-byte point in registers spills

// digit records of one scalar vector, split by bucket range; shared by every table over those scalars
// nbat vectors of n scalars end to end (fused batch; nbat = 1: one proof)
// cleared: the kernel in front of this call on the stream already zeroed the lists' counters (ingest_kernel for w, combine_h_kernel
// for h: kernels_ntt.hpp) -- the proof path; the stage hooks clear them with a memset of their own
static int msm_digits_enqueue(Prof pf, hipStream_t s, const Fr *scalars, uint32_t n_per, int nbat, const MsmPlan &pl, const DigitLists &dl, bool cleared = false) {
  if (n_per == 0) return 0;
  const uint32_t n = n_per * (uint32_t)nbat, nR = pl.nR * (uint32_t)nbat;
  int nbl_log = 0;
  while ((1u << nbl_log) < pl.nbl) nbl_log++;
  int sp = prof_begin(pf, s, "msm_sort");
  if (!cleared) ZKR_HIP_CHECK(hipMemsetAsync(dl.rng, 0, DIGIT_CLEAR_WORDS * 4, s));
  // scalars per thread (kernels_msm.hpp, stage 1): four from 2^18 scalars on; the staged scatter takes what its LDS stage holds
  int spt = n >= (1u << 18) ? 4 : n >= (1u << 17) ? 2 : 1;
  const uint32_t per_scalar = (uint32_t)pl.K * MSM_THREADS;
  const bool staged = per_scalar <= DIGIT_STAGE;
  if (staged && (uint32_t)spt * per_scalar > DIGIT_STAGE) spt = (int)(DIGIT_STAGE / per_scalar);
  unsigned grid = (n + MSM_THREADS * spt - 1) / (MSM_THREADS * spt);
  const uint32_t tmax = digit_spread_tmax(pl.c, pl.K);
  uint32_t *cnt = dl.rng, *fill = dl.rng + DIGIT_XCDS * MAX_RANGES, *off = dl.rng + 2 * DIGIT_XCDS * MAX_RANGES;
  msm_digits_count_kernel<<<grid, MSM_THREADS, 0, s>>>(scalars, n, n_per, pl.c, pl.K, nbl_log, pl.nR, nR, cnt, tmax, spt);
  if (staged) msm_digits_scatter_kernel<true><<<grid, MSM_THREADS, (size_t)DIGIT_STAGE * 8, s>>>(scalars, n, n_per, pl.c, pl.K, nbl_log, pl.nR, nR, cnt, fill, off, dl.ent_s, dl.ent_b, tmax, spt);
  else msm_digits_scatter_kernel<false><<<grid, MSM_THREADS, 0, s>>>(scalars, n, n_per, pl.c, pl.K, nbl_log, pl.nR, nR, cnt, fill, off, dl.ent_s, dl.ent_b, tmax, spt);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// digit sort of one table: LDS histogram per (window, chunk) -> scans -> LDS-cursor scatter
// n_scalars: scalars per proof (the records carry indices into the concatenated vectors of the batch); n: points of the table
static int msm_sort_enqueue(Prof pf, hipStream_t s, const uint32_t *rank, const DigitLists &dl, uint32_t n_scalars, uint32_t n, int nbat, const MsmPlan &pl, const MsmSort &ws) {
  int sp = prof_begin(pf, s, "msm_sort");
  const uint32_t nb = pl.nb * (uint32_t)nbat;  // the bucket sets of the batch end to end
  const unsigned sort_grid = pl.nR * (unsigned)nbat * pl.J;
  const size_t lds = (size_t)pl.nbl * 4;
  const uint32_t *rng_off = dl.rng + 2 * DIGIT_XCDS * MAX_RANGES;
  const unsigned scan_blocks = (nb + SCAN_BLOCK - 1) / SCAN_BLOCK;
  // Seven launches per table: histogram (whose first workgroup clears what the later ones accumulate into), column scan, three-launch
  // scan (+ oversized-bucket list + size classes), ordering, scatter.  A single-pass look-back scan in one launch (four launches per
  // sort) measured equal within the run-to-run spread on every rate and latency with a larger stage sum (a tile's column scan has
  // fewer threads in flight; profiles/r4_ab_prep_chain.txt: the proof is bound by its VALU work, not by the launch count of the
  // preparation chain), so the simpler kernels ship.
  const uint32_t big_thresh = nbat > 1 ? big_threshold(n, pl.K, pl.nbw, nbat) : pl.big_thresh;  // a fused launch's bulk is nbat proofs long
  msm_hist_kernel<<<sort_grid, SORT_THREADS, lds, s>>>(dl.ent_s, dl.ent_b, rng_off, rank, n_scalars, pl.nbl, pl.J, ws.chunk_cnt, SortScratch{ws.big_count, ws.size_hist});
  msm_colscan_kernel<<<(nb + MSM_THREADS - 1) / MSM_THREADS, MSM_THREADS, 0, s>>>(ws.chunk_cnt, nb, pl.nbl, pl.J, ws.counts);
  msm_scan_sums_kernel<<<scan_blocks, SCAN_THREADS, 0, s>>>(ws.counts, nb, ws.block_sums);
  msm_scan_top_kernel<<<1, 1024, 0, s>>>(ws.block_sums, scan_blocks, ws.big_count + 1);
  msm_scan_apply_kernel<<<scan_blocks, SCAN_THREADS, 0, s>>>(ws.counts, ws.block_sums, ws.big_count + 1, ws.offsets, nb, big_thresh,
                                                            ws.big_list, ws.big_count, BIG_CAP, ws.size_hist);
  msm_order_kernel<<<scan_blocks, SCAN_THREADS, 0, s>>>(ws.counts, nb, ws.size_hist, ws.size_hist + SIZE_BINS, ws.order);
  msm_scatter_kernel<<<sort_grid, SORT_THREADS, lds, s>>>(dl.ent_s, dl.ent_b, rng_off, rank, n_scalars, n, pl.nbl, pl.J, ws.chunk_cnt, ws.offsets, ws.entries);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// The launch helpers below take the group as a bit (g2: the table's, or its chain's) and choose the kernels' field once, here.
// bucket accumulation of one point table over a finished sort (`srt` may belong to another table with the same point set: B1 and
// B2 share one); `buckets`: where the sums land (the table's set of its chain: the chain's only one, a set behind another table's,
// or -- ACC_ONTO -- a set that already holds another table's sums)
template <class F>
static void msm_accum_launch(hipStream_t s, const void *pts, uint32_t nb, const MsmSort &srt, void *buckets, int onto) {
  // small bucket sets: several lanes per bucket (kernels_msm.hpp msm_accum_split_kernel).
  // lanes per bucket by bucket count, from single-proof latencies: 2^11 / 2^13 / 2^15 buckets (circuits of 2^12 / 2^14 / 2^16):
  // 1.52 / 1.31 / 1.33, 1.83 / 1.64 / 1.68, 1.76 / 1.69 / 2.00 ms at 2 / 4 / 8 lanes; the tx circuit's 2^16 buckets: 2.30 / 2.02 /
  // 2.15 / 2.52 ms at 1 / 2 / 4 / 8 (and 631 against 614 unfused pipelined proofs/s at 2 / 4)
  const int split = nb <= (1u << 15) ? 4 : nb <= (1u << 17) ? 2 : 1;
  const Affine<F> *p = (const Affine<F> *)pts;
  XYZZ<F> *b = (XYZZ<F> *)buckets;
  if (split > 1) {
    const unsigned sgrid = (unsigned)(((size_t)nb * split + ACC_THREADS - 1) / ACC_THREADS);
    // (the Fq2 form is built for ONE wavefront per SIMD: its lane exchange holds two XYZZ points of 72 words, and the budget for
    // two spilled 170-200 B per lane; a tx proof measures the same either way, profiles/r4_11_tx_single_split_w_g2.txt)
    if (split == 2) msm_accum_split_kernel<F, MsmCfg<F>::SPLIT_W, 2><<<sgrid, ACC_THREADS, 0, s>>>(p, srt.offsets, srt.entries, nb, srt.counts, srt.order, b, onto);
    else msm_accum_split_kernel<F, MsmCfg<F>::SPLIT_W, 4><<<sgrid, ACC_THREADS, 0, s>>>(p, srt.offsets, srt.entries, nb, srt.counts, srt.order, b, onto);
  } else {
    // two wavefronts per SIMD for both G1 and G2 (amdgpu_waves_per_eu pins the register budget): with three G1 wavefronts the
    // other streams' kernels find no registers beside them, one loses the latency cover (HISTORY.md 7b)
    msm_accum_kernel<F, MsmCfg<F>::ACC_W, MsmCfg<F>::ACC_AHEAD><<<(nb + ACC_THREADS - 1) / ACC_THREADS, ACC_THREADS, 0, s>>>(p, srt.offsets, srt.entries, nb, srt.counts, srt.order, b, onto);
  }
}
static int msm_accum_enqueue(Prof pf, hipStream_t s, bool g2, const void *pts, int nbat, const MsmPlan &pl, const MsmSort &srt, void *buckets, int onto = 0) {
  const uint32_t nb = pl.nb * (uint32_t)nbat;
  int sp = prof_begin(pf, s, g2 ? MsmCfg<Fq2>::ACC_STAGE : MsmCfg<Fq>::ACC_STAGE);
  if (g2) msm_accum_launch<Fq2>(s, pts, nb, srt, buckets, onto);
  else msm_accum_launch<Fq>(s, pts, nb, srt, buckets, onto);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// oversized buckets (digit +-1 of 0/1-heavy witnesses): needs only the sort, so it runs beside the table's accumulation
template <class F>
static void msm_big_launch(hipStream_t s, const void *pts, const MsmSort &srt, void *partials) {
  msm_big_kernel<F><<<BIG_SLOTS * BIG_SPLIT, MSM_THREADS, MSM_THREADS * sizeof(XYZZ<F>), s>>>((const Affine<F> *)pts, srt.offsets, srt.entries, srt.big_list, srt.big_count,
                                                                                                             BIG_CAP, (XYZZ<F> *)partials);
}
static int msm_big_enqueue(Prof pf, hipStream_t s, bool g2, const void *pts, const MsmSort &srt, void *partials) {
  int sp = prof_begin(pf, s, "msm_big");
  if (g2) msm_big_launch<Fq2>(s, pts, srt, partials);
  else msm_big_launch<Fq>(s, pts, srt, partials);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// big-bucket partial sums -> buckets (onto: added to what the bucket holds, the other table of a shared bucket set)
static int msm_big_finish_enqueue(Prof pf, hipStream_t s, bool g2, const MsmSort &srt, const void *partials, void *buckets, bool onto = false) {
  int sp = prof_begin(pf, s, "msm_big");
  if (g2) msm_big_finish_kernel<Fq2><<<BIG_CAP / 64, 64, 0, s>>>((const G2XYZZ *)partials, srt.big_list, srt.big_count, BIG_CAP, (G2XYZZ *)buckets, onto ? 1 : 0);
  else msm_big_finish_kernel<Fq><<<BIG_CAP / 64, 64, 0, s>>>((const G1XYZZ *)partials, srt.big_list, srt.big_count, BIG_CAP, (G1XYZZ *)buckets, onto ? 1 : 0);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}
template <class F>
static void msm_reduce_launch(hipStream_t s, const MsmGeom &g, uint32_t ngroups, uint32_t ntask, const MsmChain &ch) {
  msm_reduce1_kernel<F><<<(ngroups + MSM_THREADS - 1) / MSM_THREADS, MSM_THREADS, 0, s>>>((const XYZZ<F> *)ch.buckets, g, (XYZZ<F> *)ch.group_out);
  msm_reduce2_kernel<F><<<dim3(ntask * g.S, g.batch), MSM_THREADS, MSM_THREADS * sizeof(XYZZ<F>), s>>>((const XYZZ<F> *)ch.group_out, g, (XYZZ<F> *)ch.task_out);
  msm_reduce3_kernel<F><<<g.batch, MSM_THREADS, MSM_THREADS * sizeof(XYZZ<F>), s>>>((const XYZZ<F> *)ch.task_out, g, (XYZZ<F> *)ch.result);
}
// bucket reduction of a chain -> its result points in ch.h_result: short launches of few, long-running wavefronts (raised wave
// priority), meant to run beside the next table's accumulation.  nbat: proofs fused into the launches; the chain's sets: bucket sets
// per proof that ONE launch set walks end to end (2: A's sets behind B1's) -- the group-size rules below key on the fused proofs only.
static int msm_reduce_enqueue(Prof pf, hipStream_t s, int nbat, const MsmPlan &pl, const MsmChain &ch, bool latency = false) {
  const int sets = (int)ch.sets;
  // Group size of a FUSED launch: the plan's groups keep about 2^14 of them per proof, which is what a single proof of a small
  // circuit needs to fill the chip (msm_plan); nbat proofs in one launch bring nbat times the groups, so they take larger ones --
  // about 2^15 groups per launch -- and reduce2 / reduce3 have that much less to sum: the tx circuit in batches of eight 1 063 /
  // 1 149 / 1 192 / 1 185 proofs/s at groups of 4 / 8 / 16 / 32 (tools/sweep_tx_fused_glog.sh).  The buffers are sized for the
  // plan's (smaller) groups.
  int glog = pl.glog;
  uint32_t S = pl.S;
  // Latency mode: the LAST chain of a proof that has nothing in flight beside it (a synchronous caller's proof: the other slot is
  // idle) is pure latency -- 62 dependent additions per thread in reduce1 at groups of 32 buckets.  Groups of 8 make that 14,
  // for four times the group results in reduce2 (8 additions + the tree per thread instead of 2): 0.41 + 0.11 -> ~0.10 + 0.15 ms
  // at 2^19 buckets.  It costs 0.7 % more field multiplications, so chains that run under an accumulation keep the large groups.
  if (latency && nbat == 1 && sets == 1 && glog > LAT_GLOG) {
    glog = LAT_GLOG;
    const uint32_t ng = pl.nbw >> glog, ntask = (uint32_t)(pl.c - 1 - glog) + 2;
    S = (ng + 2047) / 2048;
    if (S > 16) S = 16;
    if (S > MSM_THREADS / ntask) S = MSM_THREADS / ntask;
    if (S < 1) S = 1;
  }
  if (nbat > 1) {
    int lg = 0;
    while (((uint64_t)1 << lg) < (uint64_t)pl.nbw * (uint64_t)nbat) lg++;
    int want = lg - 15;
    if (want > 5) want = 5;
    if (want > pl.c - 1) want = pl.c - 1;
    if (want > glog) {
      glog = want;
      const uint32_t ng = pl.nbw >> glog;
      uint32_t s2 = (ng + 2047) / 2048;
      S = s2 < 1 ? 1 : s2 > pl.S ? pl.S : s2;
    }
  }
  const int nset = nbat * sets;  // bucket sets of the launch, end to end
  MsmGeom g;
  g.c = pl.c; g.K = pl.K; g.nbw = pl.nbw; g.glog = glog; g.S = S; g.batch = (uint32_t)nset;
  int sp = prof_begin(pf, s, "msm_reduce");
  uint32_t ngroups = (pl.nbw >> glog) * (uint32_t)nset;
  uint32_t ntask = (uint32_t)(pl.c - 1 - glog) + 2;
  if (ch.g2) msm_reduce_launch<Fq2>(s, g, ngroups, ntask, ch);
  else msm_reduce_launch<Fq>(s, g, ngroups, ntask, ch);
  prof_end(pf, s, sp);
  ZKR_HIP_CHECK(hipMemcpyAsync(ch.h_result, ch.result, (ch.g2 ? sizeof(G2XYZZ) : sizeof(G1XYZZ)) * nset, hipMemcpyDeviceToHost, s));
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

// stage-hook path: one table with its own scalars (n_scalars of them; rank maps scalars to kept points) on a scratch of its own
static int msm_enqueue(Prof pf, hipStream_t s, bool g2, const void *pts, const uint32_t *rank, const Fr *scalars, uint32_t n_scalars, uint32_t n,
                       const MsmPlan &pl, const MsmScratch &m) {
  int rc;
  if ((rc = msm_digits_enqueue(pf, s, scalars, n_scalars, 1, pl, m.dig))) return rc;
  if ((rc = msm_sort_enqueue(pf, s, rank, m.dig, n_scalars, n, 1, pl, m.sort))) return rc;
  if ((rc = msm_big_enqueue(pf, s, g2, pts, m.sort, m.big_partials))) return rc;
  if ((rc = msm_accum_enqueue(pf, s, g2, pts, 1, pl, m.sort, m.chain.buckets))) return rc;
  if ((rc = msm_big_finish_enqueue(pf, s, g2, m.sort, m.big_partials, m.chain.buckets))) return rc;
  return msm_reduce_enqueue(pf, s, 1, pl, m.chain);
}

static int draw_blinding(uint8_t out[32]) {
  uint32_t v[8];
  do {
    if (int rc = os_random(out, 32)) return rc;
    out[31] &= 0x3f;
    memcpy(v, out, 32);
  } while (!words_below(v, FrParams::P));
  return 0;
}
// r and s of one proof: the caller's, checked (both or neither), or drawn
static int take_blinding(const uint8_t *r32, const uint8_t *s32, uint8_t rb[32], uint8_t sb[32]) {
  if ((r32 == nullptr) != (s32 == nullptr)) { set_error("pass both r and s or neither"); return ZKR_ERR_ARG; }
  if (!r32) {
    int rc;
    if ((rc = draw_blinding(rb)) || (rc = draw_blinding(sb))) return rc;
    return 0;
  }
  memcpy(rb, r32, 32); memcpy(sb, s32, 32);
  uint32_t rv[8], sv[8];
  memcpy(rv, rb, 32); memcpy(sv, sb, 32);
  if (!words_below(rv, FrParams::P) || !words_below(sv, FrParams::P)) { set_error("blinding scalar >= r"); return ZKR_ERR_ARG; }
  return 0;
}

static int prove_submit_enqueue(zkr_key *k, ProofSlot &sl, const Fr *const *d_wsrcs, int nbat, const uint8_t *r32s, const uint8_t *s32s, hipStream_t caller, const hipEvent_t *readies,
                                bool coefficients = false);

// Enqueue the whole GPU side of one proof on the slot's buffers; returns without waiting.  If the enqueue fails part
// way, kernels already launched still use the slot's buffers while the slot stays marked free: the key's streams are
// drained before the error is returned, so the next submit (possibly from another host thread) cannot race with them.
// nbat witnesses (1 <= nbat <= sl.cap: a fused batch shares every launch); r32s / s32s: nbat x 32 B or both
// null (drawn per proof).  readies[j]: the event after which witness j is in place (a staged upload); readies == null:
// whatever is enqueued on `caller` now.
// coefficients: H in coefficient form even if the key has the side tables of the evaluation form (prove_collect's second run of a
// group with a witness that does not satisfy the R1CS)
static int prove_submit_group(zkr_key *k, ProofSlot &sl, const Fr *const *d_wsrcs, int nbat, const uint8_t *r32s, const uint8_t *s32s, hipStream_t caller, const hipEvent_t *readies = nullptr,
                              bool coefficients = false) {
  int rc = prove_submit_enqueue(k, sl, d_wsrcs, nbat, r32s, s32s, caller, readies, coefficients);
  if (rc && rc != ZKR_ERR_ARG) {  // ZKR_ERR_ARG: refused before the first launch
    key_streams_sync(k);
    sl.spans.clear();
    sl.event_next = 0;
  }
  return rc;
}

static int prove_submit_enqueue(zkr_key *k, ProofSlot &sl, const Fr *const *d_wsrcs, int nbat, const uint8_t *r32s, const uint8_t *s32s, hipStream_t caller, const hipEvent_t *readies,
                                bool coefficients) {
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  const ArenaHeader &h = k->h;
  const ProofLayout &lay = k->layout;
  const unsigned char *ar = k->arena;
  const Prof pf{k, &sl};
  if (nbat < 1 || nbat > sl.cap) { set_error("a proof slot of this key takes 1..%d proofs at once, got %d", sl.cap, nbat); return ZKR_ERR_ARG; }
  for (int j = 0; j < nbat; j++)
    if (int rc = take_blinding(r32s ? r32s + 32 * j : nullptr, s32s ? s32s + 32 * j : nullptr, &sl.rb[32 * j], &sl.sb[32 * j])) return rc;
  sl.nbat = nbat;
  // The streams are the device's, shared by every key on it (zkr_key.hip DeviceStreams): the launches of one proof are enqueued
  // without another key's in between, so that every cross-stream wait below points at work enqueued before it
  std::unique_lock<std::mutex> enqueue_lock(*k->enqueue_mu);

  // The caller's stream only orders the witness before the proof (it may carry unrelated work, and with two
  // proofs in flight it must not chain them).  Schedule on the key's own streams (HIP multiplexes streams onto a
  // few hardware queues; streams sharing one serialise):
  //   sp : preparation -- ingest, digit records of w, the digit sorts of B and A (C shares A's: h.share_ac), calcH (QAP rows + six NTTs),
  //        digit records of h, the sort of H.  Memory/LDS-bound (and the NTTs), small workgroups;
  //   s  : the five bucket accumulations back to back, B2 first (its reduction chain is the longest), B1 on the
  //        same sort (h.share_b), then A, C, H, each waiting only for its table's sort.  Every accumulation
  //        saturates the VALUs on its own;
  //   g2 : oversized-bucket and reduction chain of the G2 table;  g1 : those of the four G1 tables (more
  //        streams measured slower, HISTORY.md 7b; one stream for all five chains is the bottleneck with two proofs in
  //        flight: ~6 ms of serialised launches per proof).  Few long-running wavefronts at raised wave priority
  //        that run under the following accumulations; the oversized buckets need only the sort and run beside
  //        the accumulation;
  //   aux : C's oversized buckets in a lone proof of a small circuit (c_big below), a shard's witness-side sorts (par_sorts).
  // With two proofs in flight (zkr_prove_submit) the preparation of proof i+1 runs under the accumulations of
  // proof i, whose reduction tail and host assembly are covered by the accumulations of proof i+1.
  // ZKR_SERIAL=1 (a profiling aid: isolated kernel durations) puts every role on the accumulation stream and turns off what only
  // concurrency is for: auxiliary-stream work, the split calcH, the latency-mode chain.  The same kernels then run in the same
  // order; a wait for an event of the same stream orders nothing new.
  static const bool serial = getenv("ZKR_SERIAL") != nullptr;
  const hipStream_t s = k->stream;
  const hipStream_t sp = serial ? s : k->prep_stream, s_g2 = serial ? s : k->g2_stream, s_g1 = serial ? s : k->g1_stream, aux = serial ? s : k->aux_stream;
  int rc;
  if (readies) {
    for (int j = 0; j < nbat; j++) ZKR_HIP_CHECK(hipStreamWaitEvent(sp, readies[j], 0));  // the staged uploads have landed
  } else {
    ZKR_HIP_CHECK(hipEventRecord(sl.ev_w, caller));   // the witnesses are in place
    ZKR_HIP_CHECK(hipStreamWaitEvent(sp, sl.ev_w, 0));
  }
  int tot = prof_begin(pf, sp, "total");
  int spn = prof_begin(pf, sp, "ingest");
  for (int j = 0; j < nbat; j++)  // the last one also clears the counters of w's digit records (msm_digits_enqueue below)
    ingest_kernel<<<(h.n + 255) / 256, 256, 0, sp>>>(d_wsrcs[j], sl.d_w + (size_t)j * h.n, h.n, j == nbat - 1 ? sl.dig_w.rng : nullptr, j == nbat - 1 ? DIGIT_CLEAR_WORDS : 0u);
  prof_end(pf, sp, spn);
  // part of a sharded proof whose calcH is split over the shards (calc_h_split: host barriers in the middle of this enqueue): the
  // chains of the four w tables are handed over BEFORE it, so that they run while the threads wait for one another.  Everywhere
  // else the accumulations are handed over after the whole preparation chain: started early they fill the chip's wavefront slots
  // and the preparation stream -- whose end, the sort of H, the last accumulation waits for -- waits for its dispatches
  // (HISTORY.md 7b / 13: a tx proof 2.13-2.40 against 1.98 ms, 2^20 the same).
  ShardGroup *const group = shard_group;
  const bool split_h = group && group->split_h && !serial && nbat == 1 && h.shard_parts == group->parts && h.shard_part == shard_group_part;
  // H in evaluation form: a whole-key proof, alone or in a fused group, on a key that has the side tables; a shard with side tables
  // only as part of a sharded proof whose caller has seen that EVERY shard has them (ShardGroup::eval_h: the partial sums of the
  // two forms differ shard by shard, only their sums over all shards agree).  A shard proving on its own keeps the coefficient
  // form.  C and H then gather from C' and E', which have the layouts and plans of the tables they stand in for (EvalTables): the
  // sorts, bucket sets (one per proof and table) and chains below do not change.
  const bool group_eval = group && group->eval_h && nbat == 1 && h.shard_parts == group->parts && h.shard_part == shard_group_part;
  const bool eval = k->eval.ready && !coefficients && (h.shard_parts == 1 ? !split_h : group_eval);
  sl.eval = eval;
  auto table_points = [&](int t) -> const void * { return eval && t == T_C ? k->eval.c_pts : eval && t == T_H ? k->eval.e_pts : ar + h.off_pts[t]; };
  const DigitLists *dig[N_TABLES] = {&sl.dig_w, &sl.dig_w, &sl.dig_w, &sl.dig_w, &sl.dig_h};
  const int *sort_src = lay.sort_src;
  // A shard key's proof is as long as its replicated calcH plus what follows it (digits and sort of h, H's accumulation, the
  // last chain): the digit records and sorts of w -- an eighth of a whole key's, but in FRONT of calcH on the preparation stream --
  // go to the auxiliary stream instead and run beside it.
  const bool par_sorts = h.shard_parts > 1 && !serial;
  const hipStream_t sw = par_sorts ? aux : sp;  // where w's digit records and the sorts of A, B1, B2, C are made
  if (par_sorts) {
    ZKR_HIP_CHECK(hipEventRecord(sl.ev_w, sp));  // the ingested witness (and the cleared counters of its digit records)
    ZKR_HIP_CHECK(hipStreamWaitEvent(sw, sl.ev_w, 0));
  }
  auto sort_table = [&](int t) -> int {  // a table that owns its sort; an empty one has none
    if (!h.npts[t]) return 0;
    const uint32_t *rank = h.rank_identity[t] || (eval && t == T_H) ? nullptr : (const uint32_t *)(ar + h.off_rank[t]);  // E' is in the order of its scalars
    hipStream_t st = t == T_H ? sp : sw;
    int rc = msm_sort_enqueue(pf, st, rank, *dig[t], rank_entries(h, t), h.npts[t], nbat, k->plan[t], sl.sort[t]);
    if (rc) return rc;
    ZKR_HIP_CHECK(hipEventRecord(sl.ev_sorted[t], st));
    return 0;
  };
  for (int c = 0; c < N_TABLES; c++) sl.res_pending[c] = false;
  // C's oversized-bucket sums on the auxiliary stream for ONE proof of a key that can fuse batches (the latency case; c_big below)
  const bool c_big_first = lay.flags[T_C] == ACC_ZERO_BIG && !serial && nbat == 1 && sl.cap > 1;
  // nothing else of this key in flight (the caller holds the key's lock: with_free_slot): this proof's last chain is latency
  bool alone = !serial;
  for (const ProofSlot &o : k->slot)
    if (&o != &sl && o.busy) alone = false;
  const bool early = split_h;  // (for a lone 2^20 / 2^22 proof the early hand-over measures the same: profiles/r6_16_lone_proof_early_handover.txt)
  bool big_sent[N_TABLES] = {false, false, false, false, false};  // the table's oversized-bucket sums are enqueued already (c_big below)
  // One table, where the layout (msm_plan.hpp proof_layout: the rules and their reasons) says it lands: (1) its chain's stream waits
  // for the table's sort and takes its oversized buckets (they need only the sort and run beside the accumulation), (2) the
  // accumulation on the accumulation stream, into the table's set of the chain, (3) after the chain's LAST table, on the chain's
  // stream again: every member's oversized-bucket sums into its set and ONE bucket reduction over all the sets.
  auto accum_table = [&](int t) -> int {
    if (lay.chain[t] < 0) return 0;  // an empty table
    int rc;
    const ChainLayout &cl = lay.chains[lay.chain[t]];
    const MsmChain &ch = sl.chain[lay.chain[t]];
    const hipStream_t rs = cl.g2 ? s_g2 : s_g1;
    const size_t set_bytes = (size_t)nbat * k->plan[cl.geom].nb * (cl.g2 ? sizeof(G2XYZZ) : sizeof(G1XYZZ));  // one set of the chain, the fused proofs end to end
    const void *pts = table_points(t);
    ZKR_HIP_CHECK(hipStreamWaitEvent(rs, sl.ev_sorted[sort_src[t]], 0));
    if (!big_sent[t]) {  // partial sums into the table's OWN partials buffer
      if ((rc = msm_big_enqueue(pf, rs, cl.g2, pts, sl.sort[sort_src[t]], sl.big_partials[t]))) return rc;
      if (lay.flags[t] == ACC_ZERO_BIG) ZKR_HIP_CHECK(hipEventRecord(sl.ev_h, rs));  // the first table of a shared set: its partial sums are on their way, the chain's end adds them in
    }
    ZKR_HIP_CHECK(hipStreamWaitEvent(s, sl.ev_sorted[sort_src[t]], 0));
    // Shared set (ACC_ZERO_BIG, then ACC_ONTO): the first table's accumulation clears the slots of ITS oversized buckets (their sums
    // are added after the last accumulation, so that one waits for nothing but the first, in front of it on the same stream)
    if ((rc = msm_accum_enqueue(pf, s, cl.g2, pts, nbat, k->plan[t], sl.sort[sort_src[t]], (char *)ch.buckets + lay.set[t] * set_bytes, lay.flags[t]))) return rc;
    ZKR_HIP_CHECK(hipEventRecord(sl.ev_done[t], s));
    if (!lay.last_of_chain(t)) return 0;  // reduced with the tables behind it, at the last one's turn on this stream
    // the stream is in order: the earlier members' partial sums (enqueued at their turns) are done; the accumulations ran on the one
    // accumulation stream, this table's last
    ZKR_HIP_CHECK(hipStreamWaitEvent(rs, sl.ev_done[t], 0));
    for (int i = 0; i < cl.n_members; i++) {  // a shared set: every table's oversized buckets are ADDED to what it holds
      const int u = cl.members[i];
      if (lay.flags[u] == ACC_ZERO_BIG) ZKR_HIP_CHECK(hipStreamWaitEvent(rs, sl.ev_h, 0));
      if ((rc = msm_big_finish_enqueue(pf, rs, cl.g2, sl.sort[sort_src[u]], sl.big_partials[u], (char *)ch.buckets + lay.set[u] * set_bytes, lay.flags[u] != 0))) return rc;
    }
    if ((rc = msm_reduce_enqueue(pf, rs, nbat, k->plan[cl.geom], ch, alone && cl.latency))) return rc;
    ZKR_HIP_CHECK(hipEventRecord(sl.ev_res[lay.chain[t]], rs));  // the chain's D2H copy is the last thing enqueued
    sl.res_pending[lay.chain[t]] = true;
    return 0;
  };
  auto chains = [&](std::initializer_list<int> ts) -> int {
    for (int t : ts)
      if (int rc = accum_table(t)) return rc;
    return 0;
  };
  // C shares H's bucket set and has no chain of its own: its oversized-bucket partial sums (needed by H's chain, which adds them
  // to the shared set) normally take C's turn on a G1 chain's stream.  There they wait for the chains in front of them: in a
  // single tx proof they ran after H's accumulation had ended, and the proof's last reduction chain started 0.2 ms late
  // (profiles/r3_07_timeline_one_tx_proof.txt).  For ONE proof of a small circuit (a key that can fuse batches, called with a
  // single witness: the latency case) they go to the auxiliary stream right behind C's sort: 2.12-2.16 against 2.16-2.24 ms per
  // tx proof.  Fused batches and large circuits keep C's turn: a fifth active stream costs them 1.5 % / 0.3 % of their rate
  // (930-943 against 947-964 tx proofs/s, 150.5 against 151.0 at 2^20: tools/ab_c_big_tx.sh).
  auto c_big = [&]() -> int {
    if (!c_big_first) return 0;
    ZKR_HIP_CHECK(hipStreamWaitEvent(aux, sl.ev_sorted[sort_src[T_C]], 0));
    int rc = msm_big_enqueue(pf, aux, false, table_points(T_C), sl.sort[sort_src[T_C]], sl.big_partials[T_C]);
    if (rc) return rc;
    ZKR_HIP_CHECK(hipEventRecord(sl.ev_h, aux));
    big_sent[T_C] = true;
    return 0;
  };
  // preparation chain
  // a shard key (zkr_key_shard) multiplies only its sub-range of each scalar vector; a whole key: sc_lo = 0, sc_n = n / m
  if ((rc = msm_digits_enqueue(pf, sw, sl.d_w + h.sc_lo[0], h.sc_n[0], nbat, k->plan[T_A], sl.dig_w, true))) return rc;
  if ((rc = sort_table(T_B1))) return rc;
  if (!lay.share_b && (rc = sort_table(T_B2))) return rc;
  if (early && (rc = chains({T_B2, T_B1}))) return rc;
  if ((rc = sort_table(T_A))) return rc;
  if (!lay.share_ac && (rc = sort_table(T_C))) return rc;
  if (early && ((rc = c_big()) || (rc = chains({T_A, T_C})))) return rc;
  if (split_h) rc = calc_h_split(k, sl, sp, *group, shard_group_part, enqueue_lock, eval);
  else if (eval) rc = calc_h_eval(k, sl, sp, nbat);
  else rc = calc_h_device(k, sl, sp, nbat);
  if (rc) return rc;
  if ((rc = msm_digits_enqueue(pf, sp, sl.d_h + h.sc_lo[1], h.sc_n[1], nbat, k->plan[T_H], sl.dig_h, true))) return rc;
  if ((rc = sort_table(T_H))) return rc;
  // accumulations + reduction chains: B2 first (its chain is the longest), one launch per table (B1 + A + C in ONE launch measured
  // 3 % slower: the launch tails it removes are where the other streams' kernels find room, profiles/r6_03_ab_groupings.txt)
  if (early) rc = chains({T_H});
  else { if ((rc = c_big())) return rc; rc = chains({T_B2, T_B1, T_A, T_C, T_H}); }
  if (rc) return rc;
  // completion = the chain and auxiliary streams done (prove_collect waits for the events on the host).  No stream is made
  // to wait for another, so nothing of the next proof queues behind this one's tail.
  prof_end(pf, s_g1, tot);  // the proof's last table, H, belongs to a G1 chain
  const hipStream_t ends[3] = {s_g2, s_g1, aux};  // sl.ev_end's order
  for (int j = 0; j < 3; j++) ZKR_HIP_CHECK(hipEventRecord(sl.ev_end[j], ends[j]));
  sl.busy = true;
  return 0;
}

// Host assembly in two phases.  Phase 1 takes A, B1, B2 only:
//   pi_a = A + alfa + r delta;  pi_b = B2 + beta + s delta;  pi_c = C + H + s pi_a + r (B1 + beta + s delta) - r s delta
//        = C + H + s (A + alfa) + r (B1 + beta) + r s delta
// i.e. every scalar multiplication: three multiples of the key's delta (window tables) and one double multiplication of the two
// MSM results with shared doublings; it writes pi_a and pi_b and returns pi_c without C + H.  Phase 2 adds C + H.
static int assemble_ab(zkr_key *k, const G1XYZZ &A, const G1XYZZ &B1, const G2XYZZ &B2, const uint8_t *rb, const uint8_t *sb, uint8_t *proof_out, G1XYZZ &pic_part) {
  const ArenaHeader &h = k->h;
  std::call_once(k->delta_once, [&] {
    k->delta1_tab = fixed_base_table(load_g1(h.delta1));
    k->delta2_tab = fixed_base_table(load_g2(h.delta2));
  });
  const G1XYZZ alfa1 = to_xyzz(load_g1(h.alfa1)), beta1 = to_xyzz(load_g1(h.beta1));
  const G2XYZZ beta2 = to_xyzz(load_g2(h.beta2));
  U256 r = load_u256(rb), sc = load_u256(sb);
  G1XYZZ a_alfa = add_full(A, alfa1), b_beta = add_full(B1, beta1);
  G1XYZZ pia = add_full(a_alfa, fixed_base_mul(k->delta1_tab, r));
  G2XYZZ pib = add_full(add_full(B2, beta2), fixed_base_mul(k->delta2_tab, sc));
  Fr rs = mul(to_mont(load_fp<FrParams>(rb)), to_mont(load_fp<FrParams>(sb)));
  Fr rs_std = from_mont(rs);
  U256 rsu;
  memcpy(rsu.v, rs_std.v, 32);
  pic_part = add_full(double_scalar_mul(a_alfa, sc, b_beta, r), fixed_base_mul(k->delta1_tab, rsu));
  if (pia.is_inf() || pib.is_inf()) return ZKR_ERR_DEGENERATE;
  store_g1_std(proof_out, to_affine(pia));
  store_g2_std(proof_out + 64, to_affine(pib));
  return 0;
}
static int assemble_c(const G1XYZZ &CH, const G1XYZZ &pic_part, uint8_t *proof_out) {
  G1XYZZ pic = add_full(CH, pic_part);
  if (pic.is_inf()) return ZKR_ERR_DEGENERATE;
  store_g1_std(proof_out + 192, to_affine(pic));
  return 0;
}

// What a shard of a proof (zkr_key_shard) contributes: its partial sums of the four group elements the assembly needs -- A, B1,
// B2 and C + H -- as this library's XYZZ points in Montgomery form.  ZKR_PARTIAL_BYTES = 128 + 128 + 256 + 128.
struct PartialSums {
  G1XYZZ A, B1;
  G2XYZZ B2;
  G1XYZZ CH;
};
static_assert(sizeof(PartialSums) == ZKR_PARTIAL_BYTES, "the partial-sum record of zkr.h");

// Wait for the slot's GPU work, then the host assembly of each of its sl.nbat proofs (proofs_out: nbat x 256 B; a degenerate
// proof fails the whole group with its status).  partials_out != null: no assembly -- the MSM results of the (one) proof are
// handed out as they are (zkr_prove_partial).
static int prove_collect(zkr_key *k, ProofSlot &sl, uint8_t *proofs_out, PartialSums *partials_out = nullptr) {
  {
    std::lock_guard<std::mutex> lk(k->mu);
    if (!sl.busy || sl.collecting) { set_error("no proof in flight in this slot"); return ZKR_ERR_ARG; }
    sl.collecting = true;
  }
  struct Release {  // the slot is free again when this scope ends, whatever the outcome; r and s do not outlive their proofs
    zkr_key *k; ProofSlot &sl;
    ~Release() {
      explicit_bzero(sl.rb.data(), sl.rb.size()); explicit_bzero(sl.sb.data(), sl.sb.size());
      { std::lock_guard<std::mutex> lk(k->mu); sl.busy = false; sl.collecting = false; }
      k->slot_freed.notify_one();
    }
  } release{k, sl};
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  const ProofLayout &lay = k->layout;
  // Everything that needs A, B1, B2 only (assemble_ab: all the scalar multiplications) is done while the LAST chains (C, H: H's
  // sort only starts after calcH) still run on the GPU; when C + H lands, one addition and one inversion finish pi_c.
  // Single-proof latency: ~0.35 ms of host work off the critical path (with two proofs in flight it was hidden already).
  auto wait_table = [&](int t) -> int {  // for the chain the table was reduced in
    const int c = lay.chain[t];
    if (c >= 0 && sl.res_pending[c]) { ZKR_HIP_CHECK(hipEventSynchronize(sl.ev_res[c])); sl.res_pending[c] = false; }
    return 0;
  };
  // the sum of table t in proof j of the group as its chain's reduction left it in the pinned host buffer (set-major); infinity for an
  // empty table and for one that landed ONTO another's set: that table's result holds both
  auto g1_result = [&](int t, int j) {
    return lay.own_result(t) ? ((const G1XYZZ *)sl.chain[lay.chain[t]].h_result)[lay.set[t] * sl.nbat + j] : G1XYZZ::inf();
  };
  int rcw;
  std::vector<G1XYZZ> pic_part((size_t)sl.nbat);
  int status = 0;
again:
  if ((rcw = wait_table(T_A)) || (rcw = wait_table(T_B1)) || (rcw = wait_table(T_B2))) return rcw;
  for (int j = 0; j < sl.nbat; j++) {
    G1XYZZ A = g1_result(T_A, j), B1 = g1_result(T_B1, j);
    G2XYZZ B2 = lay.own_result(T_B2) ? ((const G2XYZZ *)sl.chain[lay.chain[T_B2]].h_result)[j] : G2XYZZ::inf();
    if (partials_out) { partials_out[j].A = A; partials_out[j].B1 = B1; partials_out[j].B2 = B2; continue; }
    int rc = assemble_ab(k, A, B1, B2, &sl.rb[32 * j], &sl.sb[32 * j], proofs_out + 256 * j, pic_part[j]);
    if (rc) status = rc;
  }
  if ((rcw = wait_table(T_C)) || (rcw = wait_table(T_H))) return rcw;
  for (hipEvent_t e : sl.ev_end) ZKR_HIP_CHECK(hipEventSynchronize(e));  // every stream of the slot is idle (all of it precedes the table events)
  if (k->prof_on) { std::lock_guard<std::mutex> lk(k->mu); prof_collect(k, sl); }
  // H in evaluation form stands on a o b = C w (eval_h.hpp).  The counts of rows where it fails, one per witness of the group, were
  // copied out in front of the sort of H, so they have landed with the chains.  A group with a witness that leaves rows unsatisfied
  // is proved AGAIN through the coefficient form, which is exact for every witness, in this slot (its ingested witnesses, sl.d_w +
  // j n, and blinding pairs are still here) and in its proofs' places in the caller's order; what the other slot has in flight is not
  // touched.  The WHOLE group goes again, not the failing witnesses compacted into a smaller one: a resubmit overwrites the chains'
  // pinned result buffers, so the good proofs' sums would have to be set aside first, and an unsatisfying witness is the rare case.
  // `retries` counts the witnesses that failed -- what it means for lone proofs, whatever the groups a batch was cut into.
  // A shard's count goes to its group instead (this thread's: run_sharded started it): whether the witness satisfies the system is
  // known from the counts of ALL shards, and the proof goes again on every one of them (zkr_multi.hip run_sharded).
  int n_bad = 0;
  if (sl.eval && k->h.shard_parts > 1) {
    if (shard_group && shard_group_part < shard_group->unsatisfied.size()) shard_group->unsatisfied[shard_group_part] = sl.h_bad[0];
  } else if (sl.eval)
    for (int j = 0; j < sl.nbat; j++) n_bad += sl.h_bad[j] != 0;
  if (n_bad) {
    k->eval.retries.fetch_add((uint64_t)n_bad);
    const int nbat = sl.nbat;
    const size_t bl = (size_t)nbat * 32;
    uint8_t rb[32 * MAX_FUSE], sb[32 * MAX_FUSE];
    memcpy(rb, sl.rb.data(), bl); memcpy(sb, sl.sb.data(), bl);
    const Fr *w[MAX_FUSE];
    for (int j = 0; j < nbat; j++) w[j] = sl.d_w + (size_t)j * k->h.n;
    int rc;
    {
      std::lock_guard<std::mutex> lk(k->mu);
      rc = prove_submit_group(k, sl, w, nbat, rb, sb, k->prep_stream, nullptr, true);
    }
    explicit_bzero(rb, sizeof rb); explicit_bzero(sb, sizeof sb);
    if (rc) return rc;
    status = 0;
    goto again;
  }
  for (int j = 0; j < sl.nbat && !status; j++) {
    G1XYZZ C = g1_result(T_C, j), H = g1_result(T_H, j);
    if (partials_out) { partials_out[j].CH = add_full(C, H); continue; }
    status = assemble_c(add_full(C, H), pic_part[j], proofs_out + 256 * j);
  }
  if (status) { set_error("degenerate proof element (point at infinity)"); return status; }
  return 0;
}

// ------------------------------------------------------------------ host witnesses: staging ring (zkr_internal.hpp WitnessStage)
// Takes one of the STAGE_BUFS buffers; allocates its pinned and device memory on first use.  wait: block until one is free
// -- only for callers that hold no proof slot (a caller that waits for a stage while its own groups occupy the slots
// deadlocks with a caller that holds the last stage and waits for a slot); otherwise *idx = -1 when none is free.
static int stage_acquire(zkr_key *k, int *idx, bool wait = true) {
  std::unique_lock<std::mutex> lk(k->stage_mu);
  for (;;) {
    for (int i = 0; i < STAGE_BUFS; i++) {
      WitnessStage &ws = k->stage[i];
      if (ws.busy) continue;
      if (!ws.d_w) {
        ZKR_HIP_CHECK(hipSetDevice(k->device));
        const size_t count = (size_t)k->h.n * (size_t)k->slot[0].cap;  // one fused group of witnesses
        if (!ws.ev_up)
          if (int erc = ws.ev_up.create(hipEventDisableTiming)) return erc;
        if (int arc = ws.d_w.alloc(count)) return arc;  // last: a stage with d_w set is complete
      }
      ws.busy = true;
      *idx = i;
      return 0;
    }
    if (!wait) { *idx = -1; return 0; }
    k->stage_freed.wait(lk);
  }
}
static void stage_release(zkr_key *k, int idx) {
  { std::lock_guard<std::mutex> lk(k->stage_mu); k->stage[idx].busy = false; }
  k->stage_freed.notify_one();
}
// host witness j of a group -> HBM; with `last` set ws.ev_up is recorded: it fires when the whole group has landed.
// The copy goes on the key's preparation stream (a fifth stream would share one of the four hardware queues with the
// accumulation or a reduction stream and serialise with it: 448 -> 365 proofs/s on the tx circuit when tried).  Default:
// hipMemcpyAsync straight from the caller's pageable buffer -- the runtime pins the pages and DMAs from them, about 0.5 ms
// for 32 MB, blocking only this caller thread and, unlike round 1, outside the key's lock.  (A copy into a pinned bounce buffer
// first -- 2-3 ms of memcpy per 32 MB on one thread -- was slower for a single caller: 79.9 against 93.9 proofs/s at 2^20.)
static int stage_upload(zkr_key *k, int idx, int j, const void *witness_std, size_t len, bool last) {
  WitnessStage &ws = k->stage[idx];
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  ZKR_HIP_CHECK(hipMemcpyAsync((uint8_t *)ws.d_w + (size_t)j * len, witness_std, len, hipMemcpyHostToDevice, k->prep_stream));
  if (last) ZKR_HIP_CHECK(hipEventRecord(ws.ev_up, k->prep_stream));
  return 0;
}
// Groups of a batch of `count` proofs: as few submits as the key's fused capacity allows, of sizes that differ by at most
// one -- 50 proofs at capacity 8 go as 8 + 7 x 6, not 6 x 8 + 2: a group of two costs almost the launches and latency chains
// of a group of eight.  A call that fits one group is still cut in two when it is more than half the capacity (the second
// group's preparation runs under the first's accumulations); below that one group is faster (tx circuit, capacity 8:
// 4 proofs 637 against 500 proofs/s as one group, 8 proofs 696 against 733).
static size_t group_count(const zkr_key *k, size_t count) {
  const size_t cap = (size_t)k->slot[0].cap;
  if (cap <= 1 || count <= 1) return count;
  const size_t ng = (count + cap - 1) / cap;
  return ng == 1 && 2 * count > cap ? 2 : ng;
}
static int next_group(size_t remaining, size_t groups_left) { return (int)((remaining + groups_left - 1) / groups_left); }

// Hand out a free proof slot and run `enqueue` on it under the key's lock (two host threads proving on one key --
// e.g. two libuv workers behind Promise.all -- then pipeline like submit/collect does).  wait: block until a slot
// frees instead of failing.
constexpr int NO_FREE_SLOT = 1;  // internal: with_free_slot(wait = false, quiet) found every slot in flight
template <class Fn>
static int with_free_slot(zkr_key *key, bool wait, int *ticket, Fn enqueue, bool quiet = false) {
  std::unique_lock<std::mutex> lk(key->mu);
  for (;;) {
    for (int i = 0; i < PROOF_SLOTS; i++) {
      int t = (key->next_slot + i) % PROOF_SLOTS;
      if (!key->slot[t].busy) {
        key->next_slot = (t + 1) % PROOF_SLOTS;
        int rc = enqueue(key->slot[t]);
        if (!rc && ticket) *ticket = t;
        return rc;
      }
    }
    if (!wait) {
      if (quiet) return NO_FREE_SLOT;
      set_error("all %d proof slots are in flight: collect one first", PROOF_SLOTS);
      return ZKR_ERR_ARG;
    }
    key->slot_freed.wait(lk);
  }
}
// The batch calls' way to a slot: a caller with groups in flight never WAITS for a slot (or a staging buffer) -- it collects
// its own oldest group, which frees one of each -- and blocks only while it holds nothing another caller could be waiting
// for.  (Hold-and-wait on both resources deadlocked a batch call against any other host-buffer caller of the key.)
template <class Fn, class Collect>
static int take_slot(zkr_key *key, int &in_flight, int *ticket, Fn enqueue, Collect collect_oldest) {
  for (;;) {
    int rc = with_free_slot(key, in_flight == 0, ticket, enqueue, true);
    if (rc != NO_FREE_SLOT) return rc;
    if ((rc = collect_oldest())) return rc;
  }
}

}  // namespace zkr

using namespace zkr;

// a shard key (zkr_key_shard) holds a range of every table: assembled as a proof, its sums would be a wrong proof without a sign of
// it -- the proof entry points refuse it; zkr_prove_partial / zkr_prove_sharded are its callers
static int refuse_shard(const zkr_key *key) {
  if (key->h.shard_parts <= 1) return 0;
  set_error("this key is shard %u of %u of a proving key: use zkr_prove_partial / zkr_prove_sharded", key->h.shard_part, key->h.shard_parts);
  return ZKR_ERR_ARG;
}
static int check_witness_len(const zkr_key *key, size_t witness_len) {
  if (witness_len == (size_t)key->h.n * 32) return 0;
  set_error("witness is %zu bytes, key expects nVars*32 = %zu", witness_len, (size_t)key->h.n * 32);
  return ZKR_ERR_BAD_WITNESS;
}

// Where the witnesses of a proving call are: host buffers of `len` bytes each -- a host buffer is complete when the call is made;
// it is staged (own staging buffer, uploaded outside the key's lock: concurrent callers copy in parallel and a third caller uploads
// while two proofs are in flight) -- or device memory, read after whatever is enqueued on `stream` when its proof is submitted.
struct Witnesses {
  const void *const *w;
  bool host;
  size_t len;
  hipStream_t stream;
};

// Every proving call but submit / collect: a pipeline of one host thread over groups of proofs (group_count; one proof per group
// for circuits that fill the chip alone).  The host witnesses of the next group are staged BEFORE the oldest group in flight is
// collected, i.e. while both proof slots compute; then the freed slot takes the group at once.  A single proof is a call of one:
// with nothing in flight it waits for a staging buffer and for a slot.  Out: count x 256 B of proofs, or -- partial, count = 1 --
// the MSM sums of a shard's proof, not assembled.
static int prove_pipeline(zkr_key *key, const Witnesses &src, size_t count, const uint8_t *r32s, const uint8_t *s32s, uint8_t *proofs_out,
                          PartialSums *partial = nullptr) {
  size_t groups_left = group_count(key, count);
  int tickets[PROOF_SLOTS], stages[PROOF_SLOTS];
  size_t first[PROOF_SLOTS];
  int in_flight = 0, rc = 0;
  auto collect_oldest = [&]() {
    int r = prove_collect(key, key->slot[tickets[0]], partial ? nullptr : proofs_out + 256 * first[0], partial);
    if (stages[0] >= 0) stage_release(key, stages[0]);
    for (int j = 1; j < in_flight; j++) { tickets[j - 1] = tickets[j]; first[j - 1] = first[j]; stages[j - 1] = stages[j]; }
    in_flight--;
    return r;
  };
  for (size_t i = 0; i < count && !rc;) {
    const int nb = next_group(count - i, groups_left--);
    int st = -1;
    if (src.host) {
      while (!rc && st < 0) {  // a staging buffer: without waiting while groups of this call hold slots and stages
        if ((rc = stage_acquire(key, &st, in_flight == 0)) || st >= 0) break;
        rc = collect_oldest();
      }
      if (rc) { if (st >= 0) stage_release(key, st); break; }
      for (int j = 0; j < nb && !rc; j++) rc = stage_upload(key, st, j, src.w[i + j], src.len, j == nb - 1);
    }
    if (!rc && in_flight == PROOF_SLOTS) rc = collect_oldest();
    int t = -1;
    if (!rc) rc = take_slot(key, in_flight, &t, [&](ProofSlot &sl) -> int {
      const Fr *w[MAX_FUSE];
      hipEvent_t ready[MAX_FUSE];
      for (int j = 0; j < nb; j++) {
        w[j] = st >= 0 ? key->stage[st].d_w + (size_t)j * key->h.n : (const Fr *)src.w[i + j];
        ready[j] = st >= 0 ? key->stage[st].ev_up : nullptr;
      }
      return prove_submit_group(key, sl, w, nb, r32s ? r32s + 32 * i : nullptr, s32s ? s32s + 32 * i : nullptr, st >= 0 ? key->prep_stream : src.stream,
                                st >= 0 ? ready : nullptr);
    }, collect_oldest);
    if (rc) {
      if (st >= 0) { hipStreamSynchronize(key->prep_stream); stage_release(key, st); }
      break;
    }
    tickets[in_flight] = t; first[in_flight] = i; stages[in_flight] = st; in_flight++;
    i += (size_t)nb;
  }
  while (in_flight > 0) {  // drain, also after an error: a submitted group must be collected to free its slot
    int r = collect_oldest();
    if (!rc) rc = r;
  }
  return rc;
}

// A shard proving on its own takes its shard's turn: a split group that failed on this shard set drains its stragglers (whose
// cross passes write THIS shard's vectors) before it gives the turns back (zkr_multi.hip run_shards_once).  SHARED: standalone
// partial proofs from several host threads still pipeline through the shard's two proof slots; only a split group is exclusive
static std::shared_lock<std::shared_mutex> own_turn(zkr_key *key) {
  if (key->h.shard_parts > 1 && !shard_turn_held) return std::shared_lock<std::shared_mutex>(key->split_mu);
  return std::shared_lock<std::shared_mutex>();
}
// blinding plays no part before the assembly: a shard's slot gets zeros
static const uint8_t ZERO32[32] = {0};
static int prove_partial(zkr_key *key, const Witnesses &src, uint8_t partial_out[ZKR_PARTIAL_BYTES]) {
  auto turn = own_turn(key);
  PartialSums ps;
  int rc = prove_pipeline(key, src, 1, ZERO32, ZERO32, nullptr, &ps);
  if (!rc) memcpy(partial_out, &ps, sizeof(ps));
  return rc;
}

extern "C" {

int zkr_prove_submit(zkr_key *key, const void *d_witness_std, const uint8_t *r32, const uint8_t *s32, void *stream, int *ticket) {
  if (!key || !d_witness_std || !ticket) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rs = refuse_shard(key)) return rs;
  const Fr *w = (const Fr *)d_witness_std;
  return with_free_slot(key, false, ticket, [&](ProofSlot &sl) { return prove_submit_group(key, sl, &w, 1, r32, s32, (hipStream_t)stream); });
}

int zkr_prove_collect(zkr_key *key, int ticket, uint8_t proof_out[256]) {
  if (!key || !proof_out || ticket < 0 || ticket >= PROOF_SLOTS) { set_error("bad argument"); return ZKR_ERR_ARG; }
  return prove_collect(key, key->slot[ticket], proof_out);
}

int zkr_prove_batch(zkr_key *key, const void *const *witnesses_std, size_t witness_len, size_t count, const uint8_t *r32s, const uint8_t *s32s,
                    uint8_t *proofs_out) {
  if (!key || (!witnesses_std && count) || !proofs_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rs = refuse_shard(key)) return rs;
  if (int rw = check_witness_len(key, witness_len)) return rw;
  for (size_t i = 0; i < count; i++)
    if (!witnesses_std[i]) { set_error("witness %zu is null", i); return ZKR_ERR_ARG; }
  return prove_pipeline(key, Witnesses{witnesses_std, true, witness_len, nullptr}, count, r32s, s32s, proofs_out);
}

int zkr_prove_batch_device(zkr_key *key, const void *const *d_witnesses_std, size_t count, const uint8_t *r32s, const uint8_t *s32s, void *stream,
                           uint8_t *proofs_out) {
  if (!key || (!d_witnesses_std && count) || !proofs_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rs = refuse_shard(key)) return rs;
  for (size_t i = 0; i < count; i++)
    if (!d_witnesses_std[i]) { set_error("witness %zu is null", i); return ZKR_ERR_ARG; }
  return prove_pipeline(key, Witnesses{d_witnesses_std, false, 0, (hipStream_t)stream}, count, r32s, s32s, proofs_out);
}

int zkr_prove_device(zkr_key *key, const void *d_witness_std, const uint8_t *r32, const uint8_t *s32, uint8_t proof_out[256], void *stream) {
  if (!key || !d_witness_std || !proof_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rs = refuse_shard(key)) return rs;
  return prove_pipeline(key, Witnesses{&d_witness_std, false, 0, (hipStream_t)stream}, 1, r32, s32, proof_out);
}

int zkr_prove(zkr_key *key, const void *witness_std, size_t witness_len, const uint8_t *r32, const uint8_t *s32, uint8_t proof_out[256], void *stream) {
  if (!key || !witness_std || !proof_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rs = refuse_shard(key)) return rs;
  if (int rw = check_witness_len(key, witness_len)) return rw;
  (void)stream;  // a host buffer is complete when the call is made: nothing on the caller's stream to wait for
  return prove_pipeline(key, Witnesses{&witness_std, true, witness_len, nullptr}, 1, r32, s32, proof_out);
}

// ---- intra-proof sharding: a shard key's share of ONE proof, and the assembly from all shares
int zkr_prove_partial_device(zkr_key *key, const void *d_witness_std, void *stream, uint8_t partial_out[ZKR_PARTIAL_BYTES]) {
  if (!key || !d_witness_std || !partial_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  return prove_partial(key, Witnesses{&d_witness_std, false, 0, (hipStream_t)stream}, partial_out);
}

int zkr_prove_partial(zkr_key *key, const void *witness_std, size_t witness_len, uint8_t partial_out[ZKR_PARTIAL_BYTES]) {
  if (!key || !witness_std || !partial_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rw = check_witness_len(key, witness_len)) return rw;
  return prove_partial(key, Witnesses{&witness_std, true, witness_len, nullptr}, partial_out);
}

int zkr_bench_shard_split_solo(zkr_key *shard, const void *d_witness_std, double *ms_out) {
  if (!shard || !d_witness_std || !ms_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  const ArenaHeader &h = shard->h;
  int klog = 0;
  while ((1u << klog) < h.shard_parts) klog++;
  if (h.shard_parts < 2 || h.shard_parts > 8 || (1u << klog) != h.shard_parts || (h.m >> (2 * klog)) < 64 || h.sc_n[1] != h.m >> klog || h.sc_lo[1] != h.shard_part * (h.m >> klog)) {
    set_error("not a shard whose calcH can be split (2, 4 or 8 parts, blocks of at least 64 columns per shard)");
    return ZKR_ERR_ARG;
  }
  ShardGroup g;
  g.parts = h.shard_parts;
  g.klog = klog;
  g.vecs.resize(g.parts);
  g.split_h = true;
  g.solo = true;
  uint8_t partial[ZKR_PARTIAL_BYTES];
  shard_group = &g;
  shard_group_part = h.shard_part;
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  const int rc = zkr_prove_partial_device(shard, d_witness_std, nullptr, partial);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  shard_group = nullptr;
  *ms_out = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
  return rc;
}

int zkr_prove_combine(zkr_key *key, const uint8_t *partials, size_t parts, const uint8_t *r32, const uint8_t *s32, uint8_t proof_out[256]) {
  if (!key || !partials || !proof_out || parts == 0) { set_error("null argument"); return ZKR_ERR_ARG; }
  uint8_t rb[32], sb[32];
  if (int rc = take_blinding(r32, s32, rb, sb)) return rc;
  PartialSums sum;
  memcpy(&sum, partials, sizeof(sum));
  for (size_t i = 1; i < parts; i++) {  // the one exchange step of the sharded proof: four additions per share
    PartialSums ps;
    memcpy(&ps, partials + i * sizeof(PartialSums), sizeof(ps));
    sum.A = add_full(sum.A, ps.A); sum.B1 = add_full(sum.B1, ps.B1); sum.B2 = add_full(sum.B2, ps.B2); sum.CH = add_full(sum.CH, ps.CH);
  }
  G1XYZZ pic_part;
  int rc = assemble_ab(key, sum.A, sum.B1, sum.B2, rb, sb, proof_out, pic_part);
  if (!rc) rc = assemble_c(sum.CH, pic_part, proof_out);
  explicit_bzero(rb, 32); explicit_bzero(sb, 32);
  if (rc) set_error("degenerate proof element (point at infinity)");
  return rc;
}

int zkr_calc_h(zkr_key *key, const void *witness_std, size_t witness_len, void *h_out) {
  if (!key || !witness_std || !h_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (witness_len != (size_t)key->h.n * 32) { set_error("witness length mismatch"); return ZKR_ERR_BAD_WITNESS; }
  ZKR_HIP_CHECK(hipSetDevice(key->device));
  std::unique_lock<std::mutex> lk(key->mu);
  ProofSlot *slp = nullptr;
  for (ProofSlot &cand : key->slot)
    if (!cand.busy) { slp = &cand; break; }
  if (!slp) { set_error("all proof slots are in flight"); return ZKR_ERR_ARG; }
  ProofSlot &sl = *slp;
  hipStream_t s = key->stream;
  // the raw witness lands in sl.d_h (m x 32 B, written only by the last kernel of calcH, after ingest has read it) when
  // it fits -- n <= m for every key this library builds -- and in a temporary otherwise
  Fr *raw = sl.d_h;
  DevBuf tmp;
  if (key->h.n > key->h.m) { if (int arc = tmp.alloc(witness_len)) return arc; raw = tmp.as<Fr>(); }
  ZKR_HIP_CHECK(hipMemcpyAsync(raw, witness_std, witness_len, hipMemcpyHostToDevice, s));
  ingest_kernel<<<(key->h.n + 255) / 256, 256, 0, s>>>(raw, sl.d_w, key->h.n);
  int rc = calc_h_device(key, sl, s, 1);
  if (rc) return rc;
  bitrev_copy_kernel<<<(key->h.m + 255) / 256, 256, 0, s>>>(sl.d_h, sl.ca, (int)key->h.logm);
  ZKR_HIP_CHECK(hipMemcpyAsync(h_out, sl.ca, (size_t)key->h.m * 32, hipMemcpyDeviceToHost, s));
  ZKR_HIP_CHECK(hipStreamSynchronize(s));
  if (key->prof_on) prof_collect(key, sl);
  return 0;
}

int zkr_ntt(void *data_std, unsigned logn, int inverse, int device) {
  if (!data_std || logn < 1 || logn > 27) { set_error("bad argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  if (int lrc = ntt_lds_check(device)) return lrc;
  size_t n = (size_t)1 << logn;
  DevBuf bd, bd2;
  HookNttTables tables;
  int rc;
  if ((rc = bd.alloc(n * 32)) || (rc = bd2.alloc(n * 32))) return rc;
  Fr *d = bd.as<Fr>(), *d2 = bd2.as<Fr>();
  ZKR_HIP_CHECK(hipMemcpy(d, data_std, n * 32, hipMemcpyHostToDevice));
  ingest_kernel<<<(unsigned)((n + 255) / 256), 256>>>(d, d, n);  // any 256-bit word -> below r, as the proving path does with witnesses: the passes state bounds on what they load
  rc = tables.build(logn);
  if (!rc) rc = run_ntt(nullptr, tables.view(), NttRun{.L = (int)logn, .dir = inverse ? DIF_INVERSE : DIF_FORWARD, .a = ntt_in_place(d)}, NO_PROF);  // natural -> bit-reversed
  if (!rc) {
    bitrev_copy_kernel<<<(unsigned)((n + 255) / 256), 256>>>(d, d2, (int)logn);
    if (inverse) scale_kernel<<<(unsigned)((n + 255) / 256), 256>>>(d2, n, inv(to_mont(fr_from_u64(n))));
    hipError_t e = hipMemcpy(data_std, d2, n * 32, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_error("copy back failed: %s", hipGetErrorString(e)); rc = ZKR_ERR_HIP; }
  }
  return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ zkr_selftest_ntt: one run_ntt / run_ntt_cross on host vectors
// A device vector of the NTT self test: its own allocation, a guard region of one full tile's bytes on either side of the data,
// filled with a fixed pattern and compared after the run.
constexpr size_t NTT_GUARD_BYTES = (size_t)32 << NTT_TILE_LOG;
constexpr int NTT_GUARD_FILL = 0xC3;
struct NttTestVec {
  DevBuf buf;
  size_t bytes = 0;
  void *host = nullptr;  // where the data came from, and where they go back to
  const char *name = "";
  unsigned row = 0;
  Fr *data() const { return reinterpret_cast<Fr *>(buf.as<unsigned char>() + NTT_GUARD_BYTES); }
  int upload(const char *nm, unsigned r, void *h, size_t n, bool ingest) {
    name = nm; row = r; host = h; bytes = n * 32;
    if (int rc = buf.alloc(bytes + 2 * NTT_GUARD_BYTES)) return rc;
    ZKR_HIP_CHECK(hipMemset(buf.p, NTT_GUARD_FILL, NTT_GUARD_BYTES));
    ZKR_HIP_CHECK(hipMemset(buf.as<unsigned char>() + NTT_GUARD_BYTES + bytes, NTT_GUARD_FILL, NTT_GUARD_BYTES));
    ZKR_HIP_CHECK(hipMemcpy(data(), h, bytes, hipMemcpyHostToDevice));
    if (ingest) ingest_kernel<<<(unsigned)((n + 255) / 256), 256>>>(data(), data(), n);  // below r, as zkr_ntt does: the passes state bounds on what they load
    return 0;
  }
  // the data back to the host; *guard_bad = 1 (and the message) when a guard byte is not the pattern any more
  int download(int *guard_bad) {
    ZKR_HIP_CHECK(hipMemcpy(host, data(), bytes, hipMemcpyDeviceToHost));
    std::vector<unsigned char> g(2 * NTT_GUARD_BYTES);
    ZKR_HIP_CHECK(hipMemcpy(g.data(), buf.p, NTT_GUARD_BYTES, hipMemcpyDeviceToHost));
    ZKR_HIP_CHECK(hipMemcpy(g.data() + NTT_GUARD_BYTES, buf.as<unsigned char>() + NTT_GUARD_BYTES + bytes, NTT_GUARD_BYTES, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < g.size() && !*guard_bad; i++)
      if (g[i] != NTT_GUARD_FILL) {
        const bool before = i < NTT_GUARD_BYTES;
        set_error("zkr_selftest_ntt: the guard %s vector %s (row block %u) changed: a launch wrote %zu bytes %s it", before ? "in front of" : "behind", name,
                  row, before ? NTT_GUARD_BYTES - i : i - NTT_GUARD_BYTES + 1, before ? "before" : "past");
        *guard_bad = 1;
      }
    return 0;
  }
};

extern "C" int zkr_selftest_ntt(int device, const zkr_ntt_selftest_desc *desc, void *in0, void *in1, void *out, void *in0_b, void *in1_b, void *out_b) {
  if (!desc) { set_error("zkr_selftest_ntt: null descriptor"); return ZKR_ERR_ARG; }
  const zkr_ntt_selftest_desc d = *desc;
  auto bad = [](const char *what) { set_error("zkr_selftest_ntt: %s", what); return ZKR_ERR_ARG; };
  if (d.logn < 1 || d.logn > 22) return bad("logn must be 1 .. 22");
  if (d.dif > 1 || d.inverse > 1 || d.pair > 1 || d.in_place > 1 || d.canon > 1 || d.cross > 1) return bad("dif, inverse, pair, in_place, canon and cross are 0 or 1");
  if (d.pre > 2) return bad("pre must be 0 (none), 1 (coset) or 2 (product)");
  if (d.reserved) return bad("the reserved word must be 0");
  if (d.pre != PRE_COSET && (d.coset_shift || d.coset_add)) return bad("coset_shift / coset_add need pre = 1");
  if (d.tlog > 24 || d.coset_shift > 24 || d.tlog < d.logn + d.coset_shift) return bad("tlog must be logn + coset_shift .. 24");
  if (d.coset_add >> d.coset_shift) return bad("coset_add must be below 2^coset_shift");
  if (d.nbat < 1 || ((uint64_t)d.nbat << d.logn) > (1ull << 24)) return bad("nbat must be at least 1, with nbat 2^logn at most 2^24 elements");
  const uint32_t Bk = d.cross && d.klog <= 3 ? (1u << d.logn) >> d.klog : 0;  // elements of a row block
  if (d.cross) {
    if (d.klog < 1 || d.klog > 3 || d.klog >= d.logn) return bad("klog must be 1 .. 3 and below logn");
    if (d.nbat != 1 || d.pair || d.want_lo || d.want_n || d.pre == PRE_COSET) return bad("a cross pass takes one transform, no pair, no range and no coset factors");
    if (!d.col_n || (uint64_t)d.col_lo + d.col_n > Bk) return bad("the columns must lie inside a row block of 2^(logn - klog) elements");
    const uint32_t wmask = (1u << ntt_cross_wlog((int)d.klog, d.col_n)) - 1;
    if ((d.col_lo & wmask) || (d.col_n & wmask)) return bad("col_lo and col_n must be multiples of the tile width (the largest power of two up to col_n and 2^(11 - klog))");
    if ((d.in_sub && d.in_sub != d.col_lo) || (d.out_sub && d.out_sub != d.col_lo)) return bad("in_sub and out_sub are 0 (whole blocks) or col_lo (local columns)");
    if (d.in_place && d.in_sub != d.out_sub) return bad("an in-place cross pass reads and writes the same buffers: in_sub = out_sub");
  } else if (d.klog || d.col_lo || d.col_n || d.in_sub || d.out_sub || d.canon) {
    return bad("klog, col_lo, col_n, in_sub, out_sub and canon need cross = 1");
  }
  const bool mul2 = d.pre == PRE_MUL;
  if (!in0 || (mul2 && !in1) || (!d.in_place && !out)) return bad("null vector (in0; in1 with pre = 2; out unless in place)");
  if (d.pair && (!in0_b || (mul2 && !in1_b) || (!d.in_place && !out_b))) return bad("null vector of the second transform (pair = 1)");
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  if (int lrc = ntt_lds_check(device)) return lrc;

  HookNttTables tables;
  int rc;
  if ((rc = tables.build(d.tlog))) return rc;
  const NttTables tb = tables.view();

  // the vectors: one allocation each (cross: one per row block), between guards
  const unsigned rows = d.cross ? 1u << d.klog : 1;
  const size_t n_in = d.cross ? (d.in_sub ? d.col_n : Bk) : (size_t)d.nbat << d.logn;
  const size_t n_out = d.cross ? (d.out_sub ? d.col_n : Bk) : n_in;
  std::vector<std::unique_ptr<NttTestVec>> all;
  auto load = [&](const char *name, void *host, size_t n, bool ingest, NttTestVec **set) -> int {
    for (unsigned r = 0; r < rows; r++) {
      all.emplace_back(new NttTestVec);
      set[r] = all.back().get();
      if (int lrc = set[r]->upload(name, r, (unsigned char *)host + (size_t)r * n * 32, n, ingest)) return lrc;
    }
    return 0;
  };
  NttTestVec *v_in0[8] = {}, *v_in1[8] = {}, *v_out[8] = {}, *v_in0b[8] = {}, *v_in1b[8] = {}, *v_outb[8] = {};
  if ((rc = load("in0", in0, n_in, true, v_in0))) return rc;
  if (mul2 && (rc = load("in1", in1, n_in, true, v_in1))) return rc;
  if (!d.in_place && (rc = load("out", out, n_out, false, v_out))) return rc;
  if (d.pair) {
    if ((rc = load("in0_b", in0_b, n_in, true, v_in0b))) return rc;
    if (mul2 && (rc = load("in1_b", in1_b, n_in, true, v_in1b))) return rc;
    if (!d.in_place && (rc = load("out_b", out_b, n_out, false, v_outb))) return rc;
  }
  ZKR_HIP_CHECK(hipGetLastError());

  // THE launch under test
  const NttDir dir = d.dif ? (d.inverse ? DIF_INVERSE : DIF_FORWARD) : (d.inverse ? DIT_INVERSE : DIT_FORWARD);
  if (!d.cross) {
    NttRun run;
    run.L = (int)d.logn;
    run.dir = dir;
    run.pre = (int)d.pre;
    run.nbat = (int)d.nbat;
    run.a.in0 = v_in0[0]->data();
    run.a.in1 = mul2 ? v_in1[0]->data() : nullptr;
    run.a.out = d.in_place ? v_in0[0]->data() : v_out[0]->data();
    run.b.in0 = d.pair ? v_in0b[0]->data() : nullptr;
    run.b.in1 = d.pair && mul2 ? v_in1b[0]->data() : nullptr;
    run.b.out = !d.pair ? nullptr : d.in_place ? v_in0b[0]->data() : v_outb[0]->data();
    run.want_lo = d.want_lo;
    run.want_n = d.want_n;
    run.coset_shift = d.coset_shift;
    run.coset_add = d.coset_add;
    rc = run_ntt(nullptr, tb, run, NO_PROF);
  } else {
    const Fr *r_in0[8], *r_in1[8];
    Fr *r_out[8];
    for (unsigned r = 0; r < rows; r++) {
      r_in0[r] = v_in0[r]->data();
      r_in1[r] = mul2 ? v_in1[r]->data() : nullptr;
      r_out[r] = d.in_place ? v_in0[r]->data() : v_out[r]->data();
    }
    NttCross cross;
    cross.L = (int)d.logn;
    cross.klog = (int)d.klog;
    cross.dir = dir;
    cross.pre = (int)d.pre;
    cross.canon = d.canon != 0;
    cross.rows_in0 = r_in0;
    cross.rows_in1 = mul2 ? r_in1 : nullptr;
    cross.rows_out = r_out;
    cross.in_sub = d.in_sub;
    cross.out_sub = d.out_sub;
    cross.col_lo = d.col_lo;
    cross.col_n = d.col_n;
    rc = run_ntt_cross(nullptr, tb, cross, NO_PROF);
  }
  const hipError_t e = hipDeviceSynchronize();  // also after a refused run: the vectors go with this scope
  if (rc) return rc;
  if (e != hipSuccess) { set_error("zkr_selftest_ntt: the run failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  int guard_bad = 0;
  for (auto &v : all)
    if ((rc = v->download(&guard_bad))) return rc;
  return guard_bad ? ZKR_ERR_HIP : 0;
}

template <class F>
static int msm_hook(const void *points_mont, const void *scalars_std, size_t n, uint8_t *out, int *is_inf, int device) {
  if (!points_mont || !scalars_std || !out || !is_inf) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  const size_t pb = sizeof(Affine<F>);
  const uint8_t *pts = (const uint8_t *)points_mont;
  std::vector<uint32_t> rank(n, RANK_NONE);
  uint32_t np = 0;
  std::vector<uint8_t> compact;
  for (size_t i = 0; i < n; i++) {
    bool inf = true;
    for (size_t b = 0; b < pb / 2 && inf; b++) inf = pts[i * pb + b] == 0;
    if (inf) continue;
    rank[i] = np++;
    compact.insert(compact.end(), pts + i * pb, pts + (i + 1) * pb);
  }
  XYZZ<F> res = XYZZ<F>::inf();
  if (np) {
    MsmPlan pl = msm_plan(n, np);
    constexpr bool g2 = sizeof(F) != 32;
    MsmScratch ms;
    int rc = msm_scratch_alloc(ms, n, np, pl, g2);
    if (rc) return rc;
    DevBuf bpts, brank, bsc, bsc2;
    if ((rc = bpts.alloc(compact.size() * pl.K)) || (rc = brank.alloc(n * 4)) || (rc = bsc.alloc(n * 32)) || (rc = bsc2.alloc(n * 32))) return rc;  // K window levels
    Affine<F> *d_pts = bpts.as<Affine<F>>();
    uint32_t *d_rank = brank.as<uint32_t>();
    Fr *d_sc = bsc.as<Fr>(), *d_sc2 = bsc2.as<Fr>();
    ZKR_HIP_CHECK(hipMemcpy(d_pts, compact.data(), compact.size(), hipMemcpyHostToDevice));
    ZKR_HIP_CHECK(hipMemcpy(d_rank, rank.data(), n * 4, hipMemcpyHostToDevice));
    ZKR_HIP_CHECK(hipMemcpy(d_sc, scalars_std, n * 32, hipMemcpyHostToDevice));
    if ((rc = msm_precompute(device, g2, d_pts, np, pl))) return rc;
    ingest_kernel<<<(unsigned)((n + 255) / 256), 256>>>(d_sc, d_sc2, n);
    rc = msm_enqueue(NO_PROF, nullptr, g2, d_pts, d_rank, d_sc2, (uint32_t)n, np, pl, ms);
    hipError_t e = hipDeviceSynchronize();  // also after a failed enqueue: nothing may still run on buffers that are about to go
    if (!rc && e != hipSuccess) { set_error("msm failed: %s", hipGetErrorString(e)); rc = ZKR_ERR_HIP; }
    if (rc) return rc;
    res = *(const XYZZ<F> *)ms.chain.h_result;
  }
  *is_inf = res.is_inf() ? 1 : 0;
  memset(out, 0, pb);
  if (!res.is_inf()) {
    Affine<F> a = to_affine(res);
    if constexpr (sizeof(F) == 32) store_g1_std(out, *reinterpret_cast<G1Affine *>(&a));
    else store_g2_std(out, *reinterpret_cast<G2Affine *>(&a));
  }
  return 0;
}

namespace zkr {
// one table of the key, either group: *out = the XYZZ sum as the chain's pinned result holds it
template <class F>
static int key_table_msm_any(const zkr_key *k, int t, const Fr *d_scalars, XYZZ<F> *out) {
  constexpr bool g2 = sizeof(F) != 32;
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  const ArenaHeader &h = k->h;
  *out = XYZZ<F>::inf();
  if (!h.npts[t]) return 0;
  MsmScratch ms;
  int rc = msm_scratch_alloc(ms, rank_entries(h, t), h.npts[t], k->plan[t], g2);
  if (rc) return rc;
  rc = msm_enqueue(NO_PROF, nullptr, g2, k->arena + h.off_pts[t], (const uint32_t *)(k->arena + h.off_rank[t]), d_scalars,
                   rank_entries(h, t), h.npts[t], k->plan[t], ms);
  hipError_t e = hipDeviceSynchronize();  // also after a failed enqueue: the workspace goes with this scope
  if (!rc && e != hipSuccess) { set_error("msm over a key table failed: %s", hipGetErrorString(e)); rc = ZKR_ERR_HIP; }
  if (rc) return rc;
  *out = *(const XYZZ<F> *)ms.chain.h_result;
  return 0;
}
int key_table_msm(const zkr_key *k, int t, const Fr *d_scalars, G1XYZZ *out) {
  if (t == T_B2) { set_error("key_table_msm: G1 tables only"); return ZKR_ERR_ARG; }
  return key_table_msm_any<Fq>(k, t, d_scalars, out);
}
int key_table_msm_g2(const zkr_key *k, const Fr *d_scalars, G2XYZZ *out) { return key_table_msm_any<Fq2>(k, T_B2, d_scalars, out); }

// The audit's transforms run with tables built for the call, never with the key's: the twiddle sections of an arena are bytes of
// whatever file the key was loaded from.
int key_twiddles_fresh_equal(const zkr_key *k, bool *same) {
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  const ArenaHeader &h = k->h;
  *same = false;
  if (h.tlog != h.logm) return 0;
  DevBuf tw, twl;
  int rc;
  if ((rc = tw.alloc((size_t)32 << h.logm)) || (rc = twl.alloc((size_t)32 << TWL_LOG))) return rc;
  ntt_twiddles_fill(tw.as<Fr>(), h.logm, twl.as<Fr>(), nullptr);  // as key_build and arena_from_base fill them
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipDeviceSynchronize());
  bool a = false, b = false;
  if ((rc = device_bytes_equal(k->device, k->arena + h.off_tw, tw.p, (size_t)32 << h.logm, &a)) || (rc = device_bytes_equal(k->device, k->arena + h.off_twl, twl.p, (size_t)32 << TWL_LOG, &b))) return rc;
  *same = a && b;
  return 0;
}
int fresh_scalar_intt(int device, unsigned logm, Fr *d_in, Fr *d_out, int nvec) {
  ZKR_HIP_CHECK(hipSetDevice(device));
  const size_t m = (size_t)1 << logm;
  HookNttTables tables;
  if (int rc = tables.build(logm)) return rc;
  if (int rc = run_ntt(nullptr, tables.view(), NttRun{.L = (int)logm, .dir = DIF_INVERSE, .nbat = nvec, .a = ntt_in_place(d_in)}, NO_PROF)) return rc;  // natural -> bit-reversed, unscaled
  for (int j = 0; j < nvec; j++) bitrev_copy_kernel<<<(unsigned)((m + 255) / 256), 256>>>(d_in + (size_t)j * m, d_out + (size_t)j * m, (int)logm);
  scale_kernel<<<(unsigned)((m * (size_t)nvec + 255) / 256), 256>>>(d_out, m * (size_t)nvec, inv(to_mont(fr_from_u64(m))));
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipDeviceSynchronize());  // the tables go with this scope
  return 0;
}

int device_points_msm(int device, bool g2, const void *d_points, uint32_t n, const Fr *const *d_scalars, int n_sums, void *out_xyzz) {
  ZKR_HIP_CHECK(hipSetDevice(device));
  const size_t pb = g2 ? sizeof(G2Affine) : sizeof(G1Affine), ob = g2 ? sizeof(G2XYZZ) : sizeof(G1XYZZ);
  const MsmPlan pl = msm_plan(n, n);
  MsmScratch ms;
  DevBuf tbl;
  int rc;
  if ((rc = msm_scratch_alloc(ms, n, n, pl, g2)) || (rc = tbl.alloc((size_t)n * pb * pl.K))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(tbl.p, d_points, (size_t)n * pb, hipMemcpyDeviceToDevice));
  if ((rc = msm_precompute(device, g2, tbl.p, n, pl))) return rc;
  for (int j = 0; j < n_sums; j++) {
    rc = msm_enqueue(NO_PROF, nullptr, g2, tbl.p, nullptr, d_scalars[j], n, n, pl, ms);
    hipError_t e = hipDeviceSynchronize();  // also after a failed enqueue: table and workspace go with this scope
    if (!rc && e != hipSuccess) { set_error("msm over a vector of points failed: %s", hipGetErrorString(e)); rc = ZKR_ERR_HIP; }
    if (rc) return rc;
    memcpy((uint8_t *)out_xyzz + (size_t)j * ob, ms.chain.h_result, ob);
  }
  return 0;
}
}  // namespace zkr

extern "C" {

int zkr_msm_g1(const void *points_mont, const void *scalars_std, size_t n, uint8_t out[64], int *is_inf, int device) {
  return msm_hook<Fq>(points_mont, scalars_std, n, out, is_inf, device);
}
int zkr_msm_g2(const void *points_mont, const void *scalars_std, size_t n, uint8_t out[128], int *is_inf, int device) {
  return msm_hook<Fq2>(points_mont, scalars_std, n, out, is_inf, device);
}

int zkr_prof_enable(zkr_key *key, int on) {
  if (!key) { set_error("null argument"); return ZKR_ERR_ARG; }
  key->prof_on = on != 0;
  return 0;
}
int zkr_prof_reset(zkr_key *key) {
  if (!key) { set_error("null argument"); return ZKR_ERR_ARG; }
  for (auto &st : key->stages) { st.ms = 0; st.launches = 0; }
  return 0;
}
int zkr_prof_get(zkr_key *key, const char *stage, double *ms_total, uint64_t *launches) {
  if (!key || !stage || !ms_total || !launches) { set_error("null argument"); return ZKR_ERR_ARG; }
  *ms_total = 0;
  *launches = 0;
  for (auto &st : key->stages)
    if (st.name == stage) { *ms_total = st.ms; *launches = st.launches; return 0; }
  if (stage_index(stage) >= 0) return 0;  // known stage, nothing recorded yet
  set_error("unknown stage '%s'", stage);
  return ZKR_ERR_ARG;
}

static int bench_fq_mul(int device, double *gmuls_per_s, int legacy) {
  if (!gmuls_per_s) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  const unsigned blocks = 256 * 8, iters = 2048;
  size_t nthreads = (size_t)blocks * MSM_THREADS;
  DevBuf buf;
  ScopedEvent ev0, ev1;
  int rc;
  if ((rc = buf.alloc(nthreads * 32)) || (rc = ev0.create()) || (rc = ev1.create())) return rc;
  Fq *d = buf.as<Fq>();
  std::vector<uint32_t> init(nthreads * 8);
  for (size_t i = 0; i < init.size(); i++) init[i] = (uint32_t)(i * 2654435761u) & ((i & 7) == 7 ? 0x0fffffffu : 0xffffffffu);
  ZKR_HIP_CHECK(hipMemcpy(d, init.data(), nthreads * 32, hipMemcpyHostToDevice));
  fq_mul_bench_kernel<<<blocks, MSM_THREADS>>>(d, 256, legacy);  // warm up: brings the clock up under this load
  float ms = 0;
  for (int rep = 0; rep < 3; rep++) {  // best of three ~30 ms launches: a single short launch scatters by +-4 % with the clock ramp
    ZKR_HIP_CHECK(hipEventRecord(ev0, nullptr));
    fq_mul_bench_kernel<<<blocks, MSM_THREADS>>>(d, (int)iters, legacy);
    ZKR_HIP_CHECK(hipEventRecord(ev1, nullptr));
    ZKR_HIP_CHECK(hipEventSynchronize(ev1));
    float t = 0;
    ZKR_HIP_CHECK(hipEventElapsedTime(&t, ev0, ev1));
    if (rep == 0 || t < ms) ms = t;
  }
  *gmuls_per_s = (double)nthreads * iters * 4 / (ms * 1e-3) / 1e9;
  return 0;
}
int zkr_selftest_f29_forms(int device, int field, int form, const uint32_t *records, size_t n, uint32_t *out) {
  if (!records || !out || form < 0 || form > 3 || (field != 0 && field != 1)) { set_error("bad argument"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  if (n == 0) return 0;
  ZKR_HIP_CHECK(hipSetDevice(device));
  Dev<uint32_t> d_in, d_out;
  int rc;
  if ((rc = d_in.alloc(n * 72)) || (rc = d_out.alloc(n * 9))) return rc;
  if (hipMemcpy(d_in, records, n * 72 * 4, hipMemcpyHostToDevice) != hipSuccess) rc = ZKR_ERR_HIP;
  if (!rc) {
    const unsigned grid = (unsigned)((n + 127) / 128);
    if (field == 0) f29_forms_kernel<Fq29><<<grid, 128>>>(d_in, n, form, d_out);
    else f29_forms_kernel<Fr29><<<grid, 128>>>(d_in, n, form, d_out);
    if (hipGetLastError() != hipSuccess || hipMemcpy(out, d_out, n * 9 * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = ZKR_ERR_HIP;
  }
  if (rc) set_error("HIP failure in the product-form self test");
  return rc;
}

int zkr_bench_fq_mul(int device, double *gmuls_per_s) { return bench_fq_mul(device, gmuls_per_s, 0); }
int zkr_bench_fq_mul_legacy(int device, double *gmuls_per_s) { return bench_fq_mul(device, gmuls_per_s, 1); }

}  // extern "C"
