// zkr_r1cs.hip -- a rank-1 constraint system resident on the device, and the check every R1CS tool chain has (`snarkjs wtns check`):
// does this witness satisfy this system, and if not, which constraint fails first (zkr_r1cs_check, zkr_r1cs_check_device).
//
// zkr_prove proves whatever witness it is given: the key holds the A and B sides of the QAP and no C side, the quotient divides
// exactly for every witness, and a violated circuit shows only in a proof no verifier accepts.  The reference's defence is
// `groth.isValid` after every proof (operator/src/snarks/common.ts:30-38), which says "invalid" and never where; its witness comes
// from `Circuit.calculateWitness` (common.ts:15-17), which checks the circuit it was compiled from and nothing a key was set up for.
//
// The system is the r1cs_bin of zkr_setup_r1cs (parse_r1cs, qap_forms.cpp): three CSR sides -- row pointers, signals, Montgomery
// coefficients as spmv_kernel takes them -- and the list of constraints with a side wider than R1CS_WIDE terms.  One launch
// evaluates the three sides of a constraint and compares a b with c in registers: no m-sized vectors exist.  The grid is
// constraints x witnesses (blockIdx.y, as spmv_kernel's fused batch).  Narrow constraints get one thread each, wide ones one
// wavefront that strides the terms over its lanes.  A witness's tallies (violated count, smallest violated index) are reduced per
// block -- wave shuffles, then LDS -- and leave it as ONE atomicAdd / atomicMin pair, the pattern of zkr_key_check.hip.
//
// Forms: a Montgomery coefficient times a standard word is standard, so a, b, c are standard.  The Montgomery product of two
// standard values is a b / 2^256, so it is compared with c / 2^256 = from_mont(c): like with like, canonical words on both sides.
//
// zkr_r1cs_matches_key ties a system to a device key by one random evaluation: see the end of the file.
#include <string.h>
#include <mutex>
#include "kernels_ntt.hpp"  // load_fr, ingest_kernel, spmv_kernel / spmv_wide_kernel (the key's own QAP evaluation, for matches_key)
#include "zkr_internal.hpp"

namespace zkr {
namespace {

constexpr uint32_t R1CS_WIDE = WIDE_ROW_TERMS;  // a constraint with a side of more terms goes to a wavefront (the key's SPMV_WIDE)
constexpr int R1CS_THREADS = 256;
constexpr size_t R1CS_CHUNK = 1024;  // witnesses per launch (gridDim.y; the limit is 65535)
constexpr unsigned long long NONE64 = ~0ull;

struct R1csSide { const uint32_t *row_ptr, *col; const Fr *coef; };
struct R1csArgs {
  R1csSide side[3];
  const uint32_t *wide;
  uint32_t n_wide, nC;
  const Fr *const *w;          // blockIdx.y -> witness (nVars x 32 B, standard form, any 256-bit words)
  unsigned long long *rep;     // blockIdx.y -> [0] violated, [1] smallest violated, [2] signal 0 is not 1
};

// a witness word as the prover uses it: below r, as ingest_kernel leaves it (2^256 < 6r)
__device__ __forceinline__ Fr load_reduced(const Fr *p) {
  Fr x = load_fr(p);
#pragma unroll 1
  for (int k = 0; k < 5; k++) x = reduce_once(x);
  return x;
}
__device__ __forceinline__ Fr side_terms(const R1csSide &sd, const Fr *w, uint32_t k0, uint32_t k1, uint32_t step) {
  Fr acc = Fr::zero();
  for (uint32_t k = k0; k < k1; k += step) acc = add(acc, mul(load_fr(sd.coef + k), load_reduced(w + sd.col[k])));
  return acc;
}
__device__ __forceinline__ bool violated(const Fr &a, const Fr &b, const Fr &c) { return !(mul(a, b) == from_mont(c)); }
__device__ __forceinline__ Fr wave_sum(Fr x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Fr y;
#pragma unroll
    for (int i = 0; i < 8; i++) y.v[i] = __shfl_xor(x.v[i], o);
    x = add(x, y);
  }
  return x;
}

// the block's tally of one witness -> one atomic pair.  Every thread of the block calls it.
__device__ void flush(unsigned long long count, unsigned long long first, unsigned long long *rep) {
  __shared__ unsigned long long s_cnt[R1CS_THREADS / 64], s_min[R1CS_THREADS / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    count += __shfl_xor(count, o);
    const unsigned long long f = __shfl_xor(first, o);
    first = f < first ? f : first;
  }
  if (threadIdx.x % 64 == 0) {
    s_cnt[threadIdx.x / 64] = count;
    s_min[threadIdx.x / 64] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c = 0, f = NONE64;
    for (unsigned w = 0; w < R1CS_THREADS / 64; w++) {
      c += s_cnt[w];
      f = s_min[w] < f ? s_min[w] : f;
    }
    if (c) {
      atomicAdd(rep, c);
      atomicMin(rep + 1, f);
    }
  }
}

__device__ __forceinline__ bool is_wide(const R1csArgs &a, uint32_t c) {
  bool wide = false;
#pragma unroll
  for (int s = 0; s < 3; s++) wide |= a.side[s].row_ptr[c + 1] - a.side[s].row_ptr[c] > R1CS_WIDE;
  return wide;
}

// one thread per constraint; the wide ones are left to r1cs_check_wide_kernel.  Thread 0 of the grid's first column also looks
// at signal 0.
static __global__ __launch_bounds__(R1CS_THREADS) void r1cs_check_kernel(R1csArgs a) {
  const Fr *w = a.w[blockIdx.y];
  unsigned long long *rep = a.rep + 3 * (size_t)blockIdx.y;
  const uint32_t c = blockIdx.x * R1CS_THREADS + threadIdx.x;
  unsigned long long count = 0, first = NONE64;
  if (c < a.nC && !is_wide(a, c)) {
    Fr v[3];
#pragma unroll
    for (int s = 0; s < 3; s++) v[s] = side_terms(a.side[s], w, a.side[s].row_ptr[c], a.side[s].row_ptr[c + 1], 1);
    if (violated(v[0], v[1], v[2])) {
      count = 1;
      first = c;
    }
  }
  if (c == 0) {
    Fr one = Fr::zero();
    one.v[0] = 1;
    if (!(load_reduced(w) == one)) rep[2] = 1;
  }
  flush(count, first, rep);
}

// wide[i] = the i-th constraint with a side wider than R1CS_WIDE: one wavefront each (four to a block), the terms of every side
// strided over the lanes, the lanes' sums added by shuffles
static __global__ __launch_bounds__(R1CS_THREADS) void r1cs_check_wide_kernel(R1csArgs a) {
  const Fr *w = a.w[blockIdx.y];
  unsigned long long *rep = a.rep + 3 * (size_t)blockIdx.y;
  const uint32_t i = blockIdx.x * (R1CS_THREADS / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
  unsigned long long count = 0, first = NONE64;
  if (i < a.n_wide) {  // uniform over the wavefront
    const uint32_t c = a.wide[i];
    Fr v[3];
#pragma unroll
    for (int s = 0; s < 3; s++) v[s] = wave_sum(side_terms(a.side[s], w, a.side[s].row_ptr[c] + lane, a.side[s].row_ptr[c + 1], 64));
    if (lane == 0 && violated(v[0], v[1], v[2])) {
      count = 1;
      first = c;
    }
  }
  flush(count, first, rep);
}

// ---- matches_key: rows [0, m) of the key's A v and B v (its own spmv kernels' output) against the system's
struct MatchArgs {
  R1csSide side[2];
  const Fr *key_eval[2];       // m words each
  const Fr *v;                 // nVars words below r
  uint32_t nC, p, m;
  unsigned long long *rep;     // [2 s] rows of side s that differ, [2 s + 1] the first
};
static __global__ __launch_bounds__(R1CS_THREADS) void r1cs_match_kernel(MatchArgs a) {
  const uint32_t c = blockIdx.x * R1CS_THREADS + threadIdx.x;
  const int s = blockIdx.y;
  unsigned long long count = 0, first = NONE64;
  if (c < a.m) {
    Fr want = Fr::zero();
    if (c < a.nC) want = side_terms(a.side[s], a.v, a.side[s].row_ptr[c], a.side[s].row_ptr[c + 1], 1);
    else if (s == 0 && c - a.nC <= a.p) want = load_fr(a.v + (c - a.nC));  // the input-consistency rows snarkjs's setup appends
    if (!(load_fr(a.key_eval[s] + c) == want)) {
      count = 1;
      first = c;
    }
  }
  flush(count, first, a.rep + 2 * s);
}

}  // namespace
}  // namespace zkr

using namespace zkr;

struct zkr_r1cs {
  int device = 0;
  uint32_t n = 0, p = 0, nC = 0, m = 0, n_wide = 0;
  uint64_t nnz[3] = {0, 0, 0};
  DevBuf rowptr[3], col[3], coef[3], wide;
  DevBuf d_ptrs, d_rep;                 // one chunk's witness pointers and reports
  PinnedBuf h_ptrs;                   // the pointers on their way up
  Pinned<unsigned long long> h_rep;   // the reports on their way down
  OwnStream stream;                   // non-blocking, the system's own
  ScopedEvent ev;                     // "the caller's stream has come this far"
  R1csSide side(int s) const { return R1csSide{rowptr[s].as<uint32_t>(), col[s].as<uint32_t>(), coef[s].as<Fr>()}; }
};

static int upload(DevBuf &d, const void *src, size_t bytes) {
  if (int rc = d.alloc(bytes)) return rc;
  if (bytes) ZKR_HIP_CHECK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

static int r1cs_upload(zkr_r1cs *cs, const Circuit &c) {
  ZKR_HIP_CHECK(hipSetDevice(cs->device));
  for (int s = 0; s < 3; s++) {
    const QapRows &q = c.side[s];
    cs->nnz[s] = q.sig.size();
    int rc;
    if ((rc = upload(cs->rowptr[s], q.rowptr.data(), q.rowptr.size() * 4)) || (rc = upload(cs->col[s], q.sig.data(), q.sig.size() * 4)) ||
        (rc = upload(cs->coef[s], q.coef.data(), q.coef.size() * sizeof(Fr))))
      return rc;
  }
  const std::vector<uint32_t> wide = wide_rows({c.side[0].rowptr.data(), c.side[1].rowptr.data(), c.side[2].rowptr.data()}, c.nC, R1CS_WIDE);
  cs->n_wide = (uint32_t)wide.size();
  if (int rc = upload(cs->wide, wide.data(), wide.size() * 4)) return rc;
  int rc;
  if ((rc = cs->d_ptrs.alloc(R1CS_CHUNK * sizeof(void *))) || (rc = cs->d_rep.alloc(R1CS_CHUNK * 3 * 8)) || (rc = cs->h_ptrs.alloc(R1CS_CHUNK * sizeof(void *))) ||
      (rc = cs->h_rep.alloc(R1CS_CHUNK * 3)) || (rc = cs->stream.create()))
    return rc;
  return cs->ev.create(hipEventDisableTiming);
}

namespace zkr {
void r1cs_view(const zkr_r1cs *cs, R1csView *v) {
  v->device = cs->device; v->n = cs->n; v->p = cs->p; v->nC = cs->nC; v->m = cs->m;
  for (int s = 0; s < 3; s++) { v->row_ptr[s] = cs->rowptr[s].as<uint32_t>(); v->col[s] = cs->col[s].as<uint32_t>(); v->coef[s] = cs->coef[s].as<Fr>(); }
  v->wide = cs->wide.as<uint32_t>(); v->n_wide = cs->n_wide; v->wide_terms = R1CS_WIDE;
}
}  // namespace zkr

extern "C" {

int zkr_r1cs_load(const void *r1cs_bin, size_t r1cs_len, int device, zkr_r1cs **out) {
  if (!r1cs_bin || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  *out = nullptr;
  Circuit c;
  if (int rc = parse_r1cs(r1cs_bin, r1cs_len, c)) return rc;  // before any device call: a malformed buffer is refused without a GPU too
  if (int rc = need_device(device)) return rc;
  zkr_r1cs *cs = new zkr_r1cs();
  cs->device = device;
  cs->n = c.n; cs->p = c.p; cs->nC = c.nC; cs->m = c.m;
  if (int rc = r1cs_upload(cs, c)) { delete cs; return rc; }
  *out = cs;
  return 0;
}

void zkr_r1cs_free(zkr_r1cs *cs) {
  if (!cs) return;
  (void)hipSetDevice(cs->device);
  delete cs;
}

int zkr_r1cs_info(const zkr_r1cs *cs, uint64_t out[6]) {
  if (!cs || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  out[0] = cs->n; out[1] = cs->p; out[2] = cs->nC;
  for (int s = 0; s < 3; s++) out[3 + s] = cs->nnz[s];
  return 0;
}

int zkr_r1cs_check_device(zkr_r1cs *cs, const void *const *d_witnesses_std, size_t count, void *stream, uint64_t *reports, int *all_satisfied) {
  if (!cs || !d_witnesses_std || !all_satisfied) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (count == 0) { set_error("no witness to check"); return ZKR_ERR_ARG; }
  for (size_t j = 0; j < count; j++)
    if (!d_witnesses_std[j]) { set_error("witness %zu is a null pointer", j); return ZKR_ERR_ARG; }
  ZKR_HIP_CHECK(hipSetDevice(cs->device));
  const hipStream_t st = cs->stream;
  ZKR_HIP_CHECK(hipEventRecord(cs->ev, (hipStream_t)stream));  // the witnesses are in place once the caller's stream has come this far
  ZKR_HIP_CHECK(hipStreamWaitEvent(st, cs->ev, 0));
  R1csArgs a;
  for (int s = 0; s < 3; s++) a.side[s] = cs->side(s);
  a.wide = cs->wide.as<uint32_t>();
  a.n_wide = cs->n_wide;
  a.nC = cs->nC;
  a.w = cs->d_ptrs.as<const Fr *>();
  a.rep = cs->d_rep.as<unsigned long long>();
  bool all = true;
  size_t bad_wit = count;  // the first witness that fails, for the message
  unsigned long long bad_rep[3] = {0, 0, 0};
  for (size_t j0 = 0; j0 < count; j0 += R1CS_CHUNK) {
    const size_t nb = count - j0 < R1CS_CHUNK ? count - j0 : R1CS_CHUNK;
    memcpy(cs->h_ptrs, d_witnesses_std + j0, nb * sizeof(void *));
    ZKR_HIP_CHECK(hipMemcpyAsync(cs->d_ptrs.p, cs->h_ptrs, nb * sizeof(void *), hipMemcpyHostToDevice, st));
    for (size_t j = 0; j < nb; j++) { cs->h_rep[3 * j] = 0; cs->h_rep[3 * j + 1] = NONE64; cs->h_rep[3 * j + 2] = 0; }
    ZKR_HIP_CHECK(hipMemcpyAsync(cs->d_rep.p, cs->h_rep, nb * 3 * 8, hipMemcpyHostToDevice, st));
    r1cs_check_kernel<<<dim3((cs->nC + R1CS_THREADS - 1) / R1CS_THREADS, (unsigned)nb), R1CS_THREADS, 0, st>>>(a);
    if (cs->n_wide) r1cs_check_wide_kernel<<<dim3((cs->n_wide + R1CS_THREADS / 64 - 1) / (R1CS_THREADS / 64), (unsigned)nb), R1CS_THREADS, 0, st>>>(a);
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpyAsync(cs->h_rep, cs->d_rep.p, nb * 3 * 8, hipMemcpyDeviceToHost, st));
    ZKR_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t j = 0; j < nb; j++) {
      const unsigned long long *r = cs->h_rep + 3 * j;
      if (reports) { reports[3 * (j0 + j)] = r[0]; reports[3 * (j0 + j) + 1] = r[1]; reports[3 * (j0 + j) + 2] = r[2]; }
      if ((r[0] || r[2]) && all) {
        all = false;
        bad_wit = j0 + j;
        memcpy(bad_rep, r, sizeof(bad_rep));
      }
    }
  }
  *all_satisfied = all ? 1 : 0;
  if (!all) {
    if (bad_rep[2] && bad_rep[0]) set_error("witness %zu: signal 0 is not 1; %llu constraints violated, first %llu", bad_wit, bad_rep[0], bad_rep[1]);
    else if (bad_rep[2]) set_error("witness %zu: signal 0 is not 1", bad_wit);
    else set_error("witness %zu: %llu constraints violated, first %llu", bad_wit, bad_rep[0], bad_rep[1]);
  }
  return 0;
}

int zkr_r1cs_check(zkr_r1cs *cs, const void *const *witnesses_std, size_t witness_len, size_t count, uint64_t *reports, int *all_satisfied) {
  if (!cs || !witnesses_std || !all_satisfied) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (count == 0) { set_error("no witness to check"); return ZKR_ERR_ARG; }
  for (size_t j = 0; j < count; j++)
    if (!witnesses_std[j]) { set_error("witness %zu is a null pointer", j); return ZKR_ERR_ARG; }
  const size_t wbytes = (size_t)cs->n * 32;
  if (witness_len != wbytes) { set_error("witness is %zu bytes, the system has %u signals (%zu bytes)", witness_len, cs->n, wbytes); return ZKR_ERR_BAD_WITNESS; }
  ZKR_HIP_CHECK(hipSetDevice(cs->device));
  // groups of at most 256 MiB of witnesses (and one chunk of pointers) through one staging buffer
  size_t group = ((size_t)256 << 20) / wbytes;
  group = group < 1 ? 1 : group > R1CS_CHUNK ? R1CS_CHUNK : group;
  group = group > count ? count : group;
  DevBuf stage;
  if (int rc = stage.alloc(group * wbytes)) return rc;
  std::vector<const void *> ptrs(group);
  for (size_t j = 0; j < group; j++) ptrs[j] = stage.as<uint8_t>() + j * wbytes;
  int all = 1;
  std::string first_msg;
  for (size_t j0 = 0; j0 < count; j0 += group) {
    const size_t nb = count - j0 < group ? count - j0 : group;
    for (size_t j = 0; j < nb; j++) ZKR_HIP_CHECK(hipMemcpy(stage.as<uint8_t>() + j * wbytes, witnesses_std[j0 + j], wbytes, hipMemcpyHostToDevice));
    int ok = 0;
    std::vector<uint64_t> rep(3 * nb);
    if (int rc = zkr_r1cs_check_device(cs, ptrs.data(), nb, nullptr, rep.data(), &ok)) return rc;
    if (reports) memcpy(reports + 3 * j0, rep.data(), rep.size() * 8);
    if (!ok && all) {
      all = 0;
      for (size_t j = 0; j < nb; j++)
        if (rep[3 * j] || rep[3 * j + 2]) {  // the message again, with the witness's index in the caller's list
          if (rep[3 * j + 2] && rep[3 * j]) set_error("witness %zu: signal 0 is not 1; %llu constraints violated, first %llu", j0 + j, (unsigned long long)rep[3 * j], (unsigned long long)rep[3 * j + 1]);
          else if (rep[3 * j + 2]) set_error("witness %zu: signal 0 is not 1", j0 + j);
          else set_error("witness %zu: %llu constraints violated, first %llu", j0 + j, (unsigned long long)rep[3 * j], (unsigned long long)rep[3 * j + 1]);
          first_msg = zkr_last_error();
          break;
        }
    }
  }
  if (!all) set_error("%s", first_msg.c_str());
  *all_satisfied = all;
  return 0;
}

// Which key a system belongs to.  nVars, nPublic and the domain agree, and for ONE random vector v of nVars field elements from the
// OS CSPRNG the key's QAP sides -- evaluated by its own spmv_kernel / spmv_wide_kernel over its arena, the way the prover reads
// them -- give, word for word: A v = the system's A v on the rows below nConstraints, v[s] on row nConstraints + s (s <= nPublic:
// the rows snarkjs's setup appends), zero above; B v = the system's on the rows below nConstraints, zero above.  Two different
// matrices agree on a random v with probability 1/r, and term order inside a row does not matter.
// It binds A and B only: the key has no C side (C reaches a key through its setup's C-query points).
int zkr_r1cs_matches_key(zkr_r1cs *cs, const zkr_key *key, int *same) {
  if (!cs || !key || !same) { set_error("null argument"); return ZKR_ERR_ARG; }
  *same = 0;
  if (cs->device != key->device) { set_error("the system is on device %d, the key on device %d", cs->device, key->device); return ZKR_ERR_ARG; }
  const ArenaHeader &h = key->h;
  if (h.n != cs->n || h.p != cs->p || h.m != cs->m) {
    set_error("the key has nVars=%u nPublic=%u domain=%u, the system nVars=%u nPublic=%u domain=%u", h.n, h.p, h.m, cs->n, cs->p, cs->m);
    return 0;
  }
  ZKR_HIP_CHECK(hipSetDevice(cs->device));
  const hipStream_t st = cs->stream;
  ZKR_HIP_CHECK(hipEventRecord(cs->ev, nullptr));  // an arena may just have been written through the null stream (zkr_key_check.hip)
  ZKR_HIP_CHECK(hipStreamWaitEvent(st, cs->ev, 0));
  const uint32_t n = cs->n, m = cs->m;
  std::vector<uint8_t> vb((size_t)n * 32);
  if (int rc = os_random(vb.data(), vb.size())) return rc;
  DevBuf d_v, d_eval, d_rep;
  int rc;
  if ((rc = upload(d_v, vb.data(), vb.size())) || (rc = d_eval.alloc((size_t)2 * m * sizeof(Fr))) || (rc = d_rep.alloc(4 * 8))) return rc;
  Fr *v = d_v.as<Fr>(), *eval[2] = {d_eval.as<Fr>(), d_eval.as<Fr>() + m};
  ingest_kernel<<<(n + 255) / 256, 256, 0, st>>>(v, v, n);  // any 256-bit word -> below r
  const unsigned char *ar = key->arena;
  SpmvSide side[2];
  for (int i = 0; i < 2; i++)
    side[i] = SpmvSide{(const uint32_t *)(ar + h.off_rowptr[i]), (const uint32_t *)(ar + h.off_col[i]), (const Fr *)(ar + h.off_coef[i]), eval[i],
                       (const uint32_t *)(ar + h.off_wide[i]), h.n_wide[i]};
  spmv_kernel<<<dim3((m + 255) / 256, 1, 2), 256, 0, st>>>(side[0], side[1], SpmvSide{}, v, m, n, 0, m, nullptr);
  const uint32_t nw = h.n_wide[0] > h.n_wide[1] ? h.n_wide[0] : h.n_wide[1];
  if (nw) spmv_wide_kernel<<<dim3(nw, 1, 2), 64, 0, st>>>(side[0], side[1], SpmvSide{}, v, m, n, 0, m);
  const unsigned long long none[4] = {0, NONE64, 0, NONE64};
  unsigned long long res[4];
  ZKR_HIP_CHECK(hipMemcpyAsync(d_rep.p, none, sizeof(none), hipMemcpyHostToDevice, st));
  MatchArgs a;
  for (int s = 0; s < 2; s++) { a.side[s] = cs->side(s); a.key_eval[s] = eval[s]; }
  a.v = v;
  a.nC = cs->nC; a.p = cs->p; a.m = m;
  a.rep = d_rep.as<unsigned long long>();
  r1cs_match_kernel<<<dim3((m + R1CS_THREADS - 1) / R1CS_THREADS, 2), R1CS_THREADS, 0, st>>>(a);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpyAsync(res, d_rep.p, sizeof(res), hipMemcpyDeviceToHost, st));
  ZKR_HIP_CHECK(hipStreamSynchronize(st));
  for (int s = 0; s < 2; s++)
    if (res[2 * s]) {
      set_error("side %c of the key differs from the system on %llu rows, first %llu", s ? 'B' : 'A', res[2 * s], res[2 * s + 1]);
      return 0;
    }
  *same = 1;
  return 0;
}

}  // extern "C"
