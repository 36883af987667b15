// zkr_key_check.hip -- what a device key's arena CONTAINS, not only its header (zkr_key_check).
//
// arena_header_fault (zkr_key.hip) proves that the sections of an arena lie where its sizes say.  The kernels then follow the
// indices stored INSIDE the sections without bounds: spmv_kernel / spmv_wide_kernel read w[col[k]] over [row_ptr[c], row_ptr[c+1])
// and take wide[i] as a row (kernels_ntt.hpp), the digit sort turns rank[s] into a point index and the accumulation gathers
// through it (kernels_msm.hpp).  Level 0 proves that every such index stays inside its section; it is cheap (the index arrays only,
// ~40 MB at 2^20) and runs on every arena that comes from outside the process (zkr_key_load_file, zkr_key_adopt_arena,
// zkr_key_adopt_base_arena).  Level 1 reads the whole arena -- every window level of every point table, the twiddles, the QAP
// coefficients -- and checks their values; it runs on request only.
//
// Every kernel is a grid-stride loop with 64-bit counts; each thread keeps a count and the smallest faulty index per section, the
// block reduces them (wave shuffles, then LDS) and adds ONE atomic per block into the section's slot of a small result record,
// which comes back to the host in one copy.  The check runs on a non-blocking stream of its own and waits for that stream only:
// proofs other threads have in flight on the device are not waited for.
#include <string.h>
#include <memory>
#include <map>
#include <mutex>
#include "eval_h.hpp"  // fr_root_of_unity
#include "kernels_msm.hpp"
#include "kernels_ntt.hpp"
#include "hostops.hpp"
#include "pairing.hpp"  // g1_on_curve / g2_on_curve / g2_in_subgroup for the header constants
#include "zkr_internal.hpp"

namespace zkr {
namespace {

constexpr int N_SEC = ZKR_KEYSEC_CONSTS + 1;
constexpr int N_PART = 5;  // QAP side (2), table (5), twiddle table (2) or header constant (5)
constexpr int CHECK_THREADS = 256;
constexpr uint64_t CHECK_MAX_BLOCKS = 2048;

// the result record: fault count and smallest faulty index per (section, part)
struct CheckRecord {
  unsigned long long count[N_SEC][N_PART];
  unsigned long long first[N_SEC][N_PART];
};

struct Tally {
  unsigned long long count = 0, first = ~0ull;
  __device__ void note(bool bad, uint64_t i) {
    if (bad) {
      count++;
      first = i < first ? i : first;
    }
  }
};

// the block's tallies of one section -> one atomic pair.  Every thread of the block calls it (the loops have no early exit).
__device__ void flush(Tally t, unsigned long long *count, unsigned long long *first) {
  __shared__ unsigned long long s_cnt[CHECK_THREADS / 64], s_min[CHECK_THREADS / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    t.count += __shfl_xor(t.count, o);
    const unsigned long long f = __shfl_xor(t.first, o);
    t.first = f < t.first ? f : t.first;
  }
  if (threadIdx.x % 64 == 0) {
    s_cnt[threadIdx.x / 64] = t.count;
    s_min[threadIdx.x / 64] = t.first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c = 0, f = ~0ull;
    for (unsigned w = 0; w < blockDim.x / 64; w++) {
      c += s_cnt[w];
      f = s_min[w] < f ? s_min[w] : f;
    }
    if (c) {
      atomicAdd(count, c);
      atomicMin(first, f);
    }
  }
  __syncthreads();  // the LDS slots serve the next flush
}

// ---- level 0: the CSR rows and the wide-row list of one QAP side (blockIdx.y)
struct CsrSide {
  const uint32_t *row_ptr, *col, *wide;
  uint32_t nnz, n_wide;
};
struct CsrArgs {
  CsrSide side[2];
  uint32_t m, n;
  CheckRecord *rec;
};
__device__ bool row_is_wide(const uint32_t *row_ptr, uint32_t c) {
  const uint32_t k0 = row_ptr[c], k1 = row_ptr[c + 1];
  return k1 >= k0 && k1 - k0 > SPMV_WIDE;
}
// row_ptr[0] == 0, row_ptr[i] <= row_ptr[i+1], row_ptr[m] == nnz (index: i); col[k] < n (index: k); wide[] strictly increasing,
// below m, every listed row wide (index: position in the list) and every wide row listed (index: the row)
static __global__ __launch_bounds__(CHECK_THREADS) void csr_check_kernel(CsrArgs a) {
  const int s = blockIdx.y;
  const CsrSide sd = a.side[s];
  const uint32_t m = a.m;
  const uint64_t span = (uint64_t)(sd.nnz > m ? sd.nnz : m) + 1;
  Tally t_rp, t_col, t_wide;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < span; i += (uint64_t)gridDim.x * blockDim.x) {
    if (i <= m) {
      const uint32_t r = sd.row_ptr[i];
      const bool bad = i == 0 ? r != 0 : false;
      t_rp.note(bad || (i < m ? r > sd.row_ptr[i + 1] : r != sd.nnz), i);
      if (i < m && row_is_wide(sd.row_ptr, (uint32_t)i)) {  // is it in the list?  (a binary search: the list is meant to be sorted)
        uint32_t lo = 0, hi = sd.n_wide;
        while (lo < hi) {
          const uint32_t mid = lo + (hi - lo) / 2;
          if (sd.wide[mid] < i) lo = mid + 1; else hi = mid;
        }
        t_wide.note(lo == sd.n_wide || sd.wide[lo] != i, i);
      }
    }
    if (i < sd.nnz) t_col.note(sd.col[i] >= a.n, i);
    if (i < sd.n_wide) {
      const uint32_t w = sd.wide[i];
      t_wide.note(w >= m || (i > 0 && sd.wide[i - 1] >= w) || !row_is_wide(sd.row_ptr, w < m ? w : 0), i);
    }
  }
  flush(t_rp, &a.rec->count[ZKR_KEYSEC_ROWPTR][s], &a.rec->first[ZKR_KEYSEC_ROWPTR][s]);
  flush(t_col, &a.rec->count[ZKR_KEYSEC_COL][s], &a.rec->first[ZKR_KEYSEC_COL][s]);
  flush(t_wide, &a.rec->count[ZKR_KEYSEC_WIDE][s], &a.rec->first[ZKR_KEYSEC_WIDE][s]);
}

// ---- the rank maps of the five tables (blockIdx.y = table).  Level 0: every entry < npts or RANK_NONE.  Level 1: the identity
// where the header says so, and equal to the twin table's map where the two share one digit sort.
struct RankArgs {
  const uint32_t *rank[N_TABLES], *twin[N_TABLES];  // twin: null unless level 1 and the table's sort is shared
  uint32_t entries[N_TABLES], npts[N_TABLES], ident[N_TABLES];  // entries = 0: the table is skipped (no points: no sort runs)
  int level;
  CheckRecord *rec;
};
static __global__ __launch_bounds__(CHECK_THREADS) void rank_check_kernel(RankArgs a) {
  const int t = blockIdx.y;
  const uint32_t *rank = a.rank[t], *twin = a.twin[t];
  const uint32_t npts = a.npts[t];
  const bool ident = a.level >= 1 && a.ident[t];
  Tally t_rank, t_val;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.entries[t]; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = rank[i];
    t_rank.note(r != RANK_NONE && r >= npts, i);
    if (a.level >= 1) t_val.note((ident && r != i) || (twin && twin[i] != r), i);
  }
  flush(t_rank, &a.rec->count[ZKR_KEYSEC_RANK][t], &a.rec->first[ZKR_KEYSEC_RANK][t]);
  flush(t_val, &a.rec->count[ZKR_KEYSEC_SHARED_RANK][t], &a.rec->first[ZKR_KEYSEC_SHARED_RANK][t]);
}

// ---- level 1: values
__device__ bool canonical_words(const Fq &x) { return words_below(x.v, FqParams::P); }
__device__ bool canonical_words(const Fq2 &x) { return words_below(x.a.v, FqParams::P) && words_below(x.b.v, FqParams::P); }
__device__ bool zero_words(const Fq &x) {
  uint32_t o = 0;
  for (int i = 0; i < 8; i++) o |= x.v[i];
  return o == 0;
}
__device__ bool zero_words(const Fq2 &x) { return zero_words(x.a) && zero_words(x.b); }
template <class PM>
__device__ bool same_limbs(const L29<PM, 2> &a, const L29<PM, 2> &b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) d |= a.v[i] ^ b.v[i];
  return d == 0;
}
__device__ bool same_limbs(const Q29<2> &a, const Q29<2> &b) { return same_limbs(a.a, b.a) && same_limbs(a.b, b.b); }

// every stored point of the table (all window levels, the form the accumulation reads: canonical coordinates x 2^261) is on
// y^2 = x^3 + b; b261 = the curve constant in that form.  All-zero points are the infinity placeholders of shared-support tables.
template <class F>
static __global__ __launch_bounds__(CHECK_THREADS) void points_check_kernel(const Affine<F> *pts, uint64_t count, F b261, unsigned long long *f_count,
                                                                            unsigned long long *f_first) {
  using C = typename CoordOf<F>::C;
  const auto b = C::template unpack<2>(b261);
  Tally tl;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
    const Affine<F> p = load_pod(pts + i);
    if (zero_words(p.x) && zero_words(p.y)) continue;
    bool ok = canonical_words(p.x) && canonical_words(p.y);
    if (ok) {  // the 29-bit forms take canonical values only (their bound is part of the type)
      const auto x = C::template unpack<2>(p.x), y = C::template unpack<2>(p.y);
      ok = same_limbs(canonical_small(sqr(y)), canonical_small(add(mul(sqr(x), x), b)));
    }
    tl.note(!ok, i);
  }
  flush(tl, f_count, f_first);
}

// QAP coefficients (Montgomery Fr, 32 B each) below r, both sides (blockIdx.y)
struct CoefArgs {
  const Fr *coef[2];
  uint32_t nnz[2];
  CheckRecord *rec;
};
static __global__ __launch_bounds__(CHECK_THREADS) void coef_check_kernel(CoefArgs a) {
  const int s = blockIdx.y;
  Tally tl;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nnz[s]; i += (uint64_t)gridDim.x * blockDim.x) {
    const Fr c = load_fr(a.coef[s] + i);
    tl.note(!words_below(c.v, FrParams::P), i);
  }
  flush(tl, &a.rec->count[ZKR_KEYSEC_COEF][s], &a.rec->first[ZKR_KEYSEC_COEF][s]);
}

// T[k] == g^k, computed exactly as twiddle_table_kernel computes it (twiddle_pow): byte equality without a scratch table
static __global__ __launch_bounds__(CHECK_THREADS) void twiddle_check_kernel(const Fr *T, uint32_t n, Fr g, unsigned long long *f_count,
                                                                             unsigned long long *f_first) {
  Tally tl;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const Fr got = load_fr(T + i), want = twiddle_pow(g, (uint32_t)i);
    uint32_t d = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) d |= got.v[j] ^ want.v[j];
    tl.note(d != 0, i);
  }
  flush(tl, f_count, f_first);
}

unsigned grid_for(uint64_t count) {
  const uint64_t b = (count + CHECK_THREADS - 1) / CHECK_THREADS;
  return (unsigned)(b < 1 ? 1 : b > CHECK_MAX_BLOCKS ? CHECK_MAX_BLOCKS : b);
}

// the curve constants in the accumulation's radix (x 2^261, canonical), from their Montgomery (x 2^256) form
Fq to261(const Fq &x) {
  Fq r;
  pack29(canonical(mul(unpack29<Fq29, 2>(x.v), const29<Fq29>(Fq29::TO261))), r.v);
  return r;
}
Fq2 to261(const Fq2 &x) { return Fq2{to261(x.a), to261(x.b)}; }

bool canonical_fq(const Fq &x) { return words_below(x.v, FqParams::P); }

// One result record (device) and its pinned host copy per device, made on first use and kept for the process (like the device's
// stream set, zkr_key.hip): a check frees nothing, and a free would wait for the whole device.  Checks on one device take turns.
struct CheckCtx {
  std::mutex mu;
  Dev<CheckRecord> d_rec;
  Pinned<CheckRecord> h_rec;
};
std::mutex g_ctx_mu;
std::map<int, CheckCtx *> g_ctx;  // never freed: a complete context lives as long as the process

const char *const SEC_NAME[N_SEC] = {"none", "rowptr", "col", "wide", "rank", "header", "points", "twiddles", "coef", "shared rank", "consts"};
const char *part_name(int sec, int part) {
  static const char *const SIDE[2] = {"side A", "side B"};
  static const char *const TABLE[N_TABLES] = {"table A", "table B1", "table B2", "table C", "table H"};
  static const char *const TW[2] = {"tw", "twl"};
  static const char *const CONST[5] = {"alfa1", "beta1", "delta1", "beta2", "delta2"};
  switch (sec) {
    case ZKR_KEYSEC_ROWPTR: case ZKR_KEYSEC_COL: case ZKR_KEYSEC_WIDE: case ZKR_KEYSEC_COEF: return SIDE[part & 1];
    case ZKR_KEYSEC_TWIDDLES: return TW[part & 1];
    case ZKR_KEYSEC_CONSTS: return CONST[part % 5];
    default: return TABLE[part % N_TABLES];
  }
}

}  // namespace

// The check of an arena whose header passed arena_header_fault (the sections lie where the sizes say): `arena` on `device`, `h`
// its header.  ZKR_OK or ZKR_ERR_BAD_KEY with the first faulty section in ZKR_KEYSEC_* order; report (may be null) as zkr_key_check.
int key_arena_check(int device, const unsigned char *arena, const ArenaHeader &h, int level, uint64_t report[4]) {
  ZKR_HIP_CHECK(hipSetDevice(device));
  CheckCtx *ctx = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    CheckCtx *&slot = g_ctx[device];
    if (!slot) {
      std::unique_ptr<CheckCtx> c(new CheckCtx());
      if (c->d_rec.alloc(1) || c->h_rec.alloc(1)) {
        set_error("key check: allocation of the result record failed");
        return ZKR_ERR_HIP;
      }
      slot = c.release();
    }
    ctx = slot;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  OwnStream os;  // the check's own non-blocking stream, destroyed when the check ends (it leaves the device's hardware queue hand-out as it was)
  if (int src = os.create()) return src;
  const hipStream_t st = os;
  {  // the arena may just have been written through the null stream (the unpacking copies of zkr_key_adopt_base_arena): wait for
     // that stream's work -- the key's own streams are non-blocking, so no proof in flight is waited for
    ScopedEvent ev;
    if (int erc = ev.create()) return erc;
    ZKR_HIP_CHECK(hipEventRecord(ev, nullptr));
    ZKR_HIP_CHECK(hipStreamWaitEvent(st, ev, 0));
  }
  CheckRecord *rec = ctx->d_rec;
  ZKR_HIP_CHECK(hipMemsetAsync(rec->count, 0, sizeof(rec->count), st));
  ZKR_HIP_CHECK(hipMemsetAsync(rec->first, 0xff, sizeof(rec->first), st));

  {
    CsrArgs a;
    for (int s = 0; s < 2; s++)
      a.side[s] = CsrSide{(const uint32_t *)(arena + h.off_rowptr[s]), (const uint32_t *)(arena + h.off_col[s]), (const uint32_t *)(arena + h.off_wide[s]),
                          s == 0 ? h.nnzA : h.nnzB, h.n_wide[s]};
    a.m = h.m;
    a.n = h.n;
    a.rec = rec;
    const uint64_t span = (uint64_t)(h.nnzA > h.nnzB ? h.nnzA : h.nnzB) + h.m + 1;
    csr_check_kernel<<<dim3(grid_for(span), 2), CHECK_THREADS, 0, st>>>(a);
  }
  {
    RankArgs a;
    uint64_t most = 0;
    const bool share_b = h.share_b && h.npts[T_B1] == h.npts[T_B2];  // the sorts zkr_prove.hip shares (prove_submit_enqueue sort_src)
    const bool share_ac = h.share_ac && h.npts[T_A] == h.npts[T_C];
    for (int t = 0; t < N_TABLES; t++) {
      a.rank[t] = (const uint32_t *)(arena + h.off_rank[t]);
      a.entries[t] = h.npts[t] ? rank_entries(h, t) : 0;
      a.npts[t] = h.npts[t];
      a.ident[t] = h.rank_identity[t];
      a.twin[t] = nullptr;
      most = a.entries[t] > most ? a.entries[t] : most;
    }
    if (level >= 1 && share_b) a.twin[T_B2] = a.rank[T_B1];
    if (level >= 1 && share_ac) a.twin[T_C] = a.rank[T_A];
    a.level = level;
    a.rec = rec;
    rank_check_kernel<<<dim3(grid_for(most), N_TABLES), CHECK_THREADS, 0, st>>>(a);
  }
  if (level >= 1) {
    const Fq b1 = to261(pairing::fq_small(3));
    const Fq2 b2 = to261(Fq2{pairing::fq_from_limbs(pairing::TWIST_B0), pairing::fq_from_limbs(pairing::TWIST_B1)});
    for (int t = 0; t < N_TABLES; t++) {
      const uint64_t count = (uint64_t)h.npts[t] * ((255 + h.win_c[t] - 1) / h.win_c[t]);
      if (!count) continue;
      unsigned long long *fc = &rec->count[ZKR_KEYSEC_POINTS][t], *ff = &rec->first[ZKR_KEYSEC_POINTS][t];
      if (t == T_B2) points_check_kernel<Fq2><<<grid_for(count), CHECK_THREADS, 0, st>>>((const G2Affine *)(arena + h.off_pts[t]), count, b2, fc, ff);
      else points_check_kernel<Fq><<<grid_for(count), CHECK_THREADS, 0, st>>>((const G1Affine *)(arena + h.off_pts[t]), count, b1, fc, ff);
    }
    twiddle_check_kernel<<<grid_for(h.m), CHECK_THREADS, 0, st>>>((const Fr *)(arena + h.off_tw), h.m, fr_root_of_unity(h.logm + 1),
                                                                   &rec->count[ZKR_KEYSEC_TWIDDLES][0], &rec->first[ZKR_KEYSEC_TWIDDLES][0]);
    twiddle_check_kernel<<<grid_for(1u << TWL_LOG), CHECK_THREADS, 0, st>>>((const Fr *)(arena + h.off_twl), 1u << TWL_LOG, fr_root_of_unity(TWL_LOG + 1),
                                                                             &rec->count[ZKR_KEYSEC_TWIDDLES][1], &rec->first[ZKR_KEYSEC_TWIDDLES][1]);
    CoefArgs c;
    for (int s = 0; s < 2; s++) {
      c.coef[s] = (const Fr *)(arena + h.off_coef[s]);
      c.nnz[s] = s == 0 ? h.nnzA : h.nnzB;
    }
    c.rec = rec;
    coef_check_kernel<<<dim3(grid_for(h.nnzA > h.nnzB ? h.nnzA : h.nnzB), 2), CHECK_THREADS, 0, st>>>(c);
  }
  ZKR_HIP_CHECK(hipGetLastError());
  CheckRecord *out = ctx->h_rec;
  ZKR_HIP_CHECK(hipMemcpyAsync(out, rec, sizeof(CheckRecord), hipMemcpyDeviceToHost, st));
  ZKR_HIP_CHECK(hipStreamSynchronize(st));

  // what the host checks itself: the header rule arena_header_fault does not make, and (level 1) the header constants
  for (int t = 0; t < N_TABLES; t++)
    if (h.rank_identity[t] && h.npts[t] != rank_entries(h, t)) {  // the sort would take scalar indices as point indices
      out->count[ZKR_KEYSEC_HEADER][t] = 1;
      out->first[ZKR_KEYSEC_HEADER][t] = h.npts[t];
    }
  if (level >= 1) {
    const uint8_t *g1s[3] = {h.alfa1, h.beta1, h.delta1};
    for (int j = 0; j < 3; j++) {
      const G1Affine p = load_g1(g1s[j]);
      if (!canonical_fq(p.x) || !canonical_fq(p.y) || !pairing::g1_on_curve(p)) { out->count[ZKR_KEYSEC_CONSTS][j] = 1; out->first[ZKR_KEYSEC_CONSTS][j] = 0; }
    }
    const uint8_t *g2s[2] = {h.beta2, h.delta2};
    for (int j = 0; j < 2; j++) {
      const G2Affine p = load_g2(g2s[j]);
      const bool canon = canonical_fq(p.x.a) && canonical_fq(p.x.b) && canonical_fq(p.y.a) && canonical_fq(p.y.b);
      if (!canon || p.is_inf() || !pairing::g2_on_curve(p) || !pairing::g2_in_subgroup(p)) { out->count[ZKR_KEYSEC_CONSTS][3 + j] = 1; out->first[ZKR_KEYSEC_CONSTS][3 + j] = 0; }
    }
  }
  for (int sec = 1; sec < N_SEC; sec++)
    for (int part = 0; part < N_PART; part++) {
      if (!out->count[sec][part]) continue;
      if (report) { report[0] = out->count[sec][part]; report[1] = (uint64_t)sec; report[2] = (uint64_t)part; report[3] = out->first[sec][part]; }
      set_error("key check: %s %s: %llu bad, first at %llu", SEC_NAME[sec], part_name(sec, part), out->count[sec][part], out->first[sec][part]);
      return ZKR_ERR_BAD_KEY;
    }
  if (report) report[0] = report[1] = report[2] = report[3] = 0;
  return 0;
}

}  // namespace zkr

extern "C" int zkr_key_check(const zkr_key *key, int level, uint64_t report[4]) {
  if (!key) { zkr::set_error("null argument"); return ZKR_ERR_ARG; }
  if (level < 0 || level > 1) { zkr::set_error("key check level %d: 0 (structure) or 1 (structure and values)", level); return ZKR_ERR_ARG; }
  return zkr::key_arena_check(key->device, key->arena, key->h, level, report);
}
