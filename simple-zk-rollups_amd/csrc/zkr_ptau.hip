// zkr_ptau.hip -- the phase-1 transcript of Bowe-Gabizon-Miers ("powers of tau"): a vector of group elements tau^i G1, tau^i G2,
// alfa tau^i G1, beta tau^i G1, beta G2 in which every contributor multiplied tau, alfa and beta by secrets of its own, so that
// nobody knows them while ONE contributor forgot its share.  zkr_setup_r1cs is a one-party setup -- its runner knows t, alfa and
// beta and can forge proofs whatever happens to delta afterwards (zkr_key_contribute) -- and a transcript is what a key nobody can
// forge for starts from.
//
// Here: the transcript's layout, the all-generators start, a contribution with its record (three Schnorr proofs, as the delta
// record's one), the check of a chain of records (host, pairings), the verification of a transcript (curve and order checks on
// the device, the progressions by random combinations through the library's MSM path), and the group elements of a key derived
// from a transcript (zkr_setup_r1cs_ptau, zkr_setup.hip): Lagrange-basis points by the inverse NTT over points, the per-signal
// sparse combinations of them, the hExps differences.  The kernels are in kernels_group.hpp; two of them are reachable on their
// own as stage hooks (zkr_points_scale_each, zkr_group_ntt).
//
// ZKRPTAU1, power K, M = 2^K (every coordinate 32 B LE standard form, G2 as x.re, x.im, y.re, y.im -- vk_bin's conventions):
//   32 B header: "ZKRPTAU1" | u32 K | u32 0 | u64 total length | 8 B zero
//   tauG1 [2M] x 64 | tauG2 [M] x 128 | alfaTauG1 [M] x 64 | betaTauG1 [M] x 64 | betaG2 128          = 160 + 384 M bytes
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "eval_h.hpp"  // fr_root_of_unity
#include "kernels_group.hpp"
#include "hostops.hpp"
#include "pairing.hpp"
#include "record_util.hpp"
#include "zkr_internal.hpp"

namespace zkr {

// ---------------------------------------------------------------- kernels of the transcript's boundary
// Standard-form coordinates -> the key's Montgomery form, in place; bad[0] counts the coordinates that are not below q (they are
// left as they are: the caller stops), bad[1] = the smallest index among them.
static __global__ void ptau_coords_in_kernel(Fq *c, size_t n, uint32_t *bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fq x = load_pod(c + i);
  if (!words_below(x.v, FqParams::P)) { group_note_bad(bad, (uint32_t)i); return; }
  store_pod(c + i, to_mont(x));
}
static __global__ void ptau_coords_out_kernel(Fq *c, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  store_pod(c + i, from_mont(load_pod(c + i)));
}

namespace {

constexpr char PTAU_MAGIC[9] = "ZKRPTAU1";
constexpr size_t PTAU_HEADER = 32;
constexpr unsigned PTAU_MAX_POWER = 24;
enum { V_TAU1 = 0, V_TAU2 = 1, V_ALFA1 = 2, V_BETA1 = 3, V_BETA2 = 4, N_VECTORS = 5 };
const char *const VECTOR_NAME[N_VECTORS] = {"tauG1", "tauG2", "alfaTauG1", "betaTauG1", "betaG2"};

struct PtauLayout {
  unsigned power;
  size_t M, total;
  size_t off[N_VECTORS], count[N_VECTORS];  // byte offsets from the start of the transcript; points
};
inline bool vector_is_g2(int v) { return v == V_TAU2 || v == V_BETA2; }
PtauLayout ptau_layout(unsigned power) {
  PtauLayout l;
  l.power = power;
  l.M = (size_t)1 << power;
  l.count[V_TAU1] = 2 * l.M; l.count[V_TAU2] = l.M; l.count[V_ALFA1] = l.M; l.count[V_BETA1] = l.M; l.count[V_BETA2] = 1;
  size_t o = PTAU_HEADER;
  for (int v = 0; v < N_VECTORS; v++) { l.off[v] = o; o += l.count[v] * (vector_is_g2(v) ? 128 : 64); }
  l.total = o;
  return l;
}
void ptau_write_header(uint8_t *out, const PtauLayout &l) {
  memset(out, 0, PTAU_HEADER);
  memcpy(out, PTAU_MAGIC, 8);
  const uint32_t k = l.power;
  const uint64_t t = l.total;
  memcpy(out + 8, &k, 4);
  memcpy(out + 16, &t, 8);
}
// null when the header and the length agree (step 1 of the verification)
const char *ptau_header_fault(const void *ptau, size_t len, PtauLayout &l) {
  if (len < PTAU_HEADER) return "shorter than its header";
  const uint8_t *b = (const uint8_t *)ptau;
  if (memcmp(b, PTAU_MAGIC, 8) != 0) return "not a ZKRPTAU1 transcript (magic)";
  uint32_t k, zero;
  uint64_t total;
  memcpy(&k, b + 8, 4); memcpy(&zero, b + 12, 4); memcpy(&total, b + 16, 8);
  if (k < 1 || k > PTAU_MAX_POWER) return "power outside 1..24";
  l = ptau_layout(k);
  static const uint8_t z8[8] = {0};
  if (zero != 0 || memcmp(b + 24, z8, 8) != 0) return "reserved header bytes are not zero";
  if (total != l.total || len != l.total) return "length does not match the power";
  return nullptr;
}

// ---------------------------------------------------------------- launches
// pts[i] <- s[i] pts[i] on the current device; d_scalars: standard form, one per point (sc_stride 1) or one for all (0);
// ztmp: 2 n coordinates
template <class C>
int scale_each_launch(Affine<typename C::W> *pts, size_t n, const Fr *d_scalars, uint32_t sc_stride, void *ztmp) {
  if (!n) return 0;
  int npt;
  const unsigned grid = group_scale_grid(n, &npt);
  group_scale_each_kernel<C><<<grid, GROUP_THREADS>>>(pts, (uint32_t)n, npt, (const uint32_t *)d_scalars, sc_stride, (typename C::W *)ztmp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

Fr fr_small(uint64_t x) {
  Fr r = Fr::zero();
  r.v[0] = (uint32_t)x; r.v[1] = (uint32_t)(x >> 32);
  return to_mont(r);
}

// NTT of n = 2^logn points on the current device, natural order in and out (oracle/groth16.py ntt's convention, which is
// zkr_ntt's): bit reversal into `tmp`, logn butterfly launches, the result back in `pts`; the inverse ends with every point
// times 1 / n (one scalar for all lanes).  tmp: n points; ztmp: 2 n coordinates; tw: n / 2 + 1 scalars.
template <class C>
int group_ntt_launch(Affine<typename C::W> *pts, Affine<typename C::W> *tmp, unsigned logn, bool inverse, Fr *tw, void *ztmp) {
  using W = typename C::W;
  const size_t n = (size_t)1 << logn;
  const uint32_t half_n = (uint32_t)(n / 2);
  Fr g = fr_root_of_unity(logn);
  if (inverse) g = inv(g);
  twiddle_table_kernel<<<(half_n + 255) / 256, 256>>>(tw, half_n, g);
  fr_to_std_kernel<<<(half_n + 255) / 256, 256>>>(tw, half_n);
  group_bitrev_kernel<W><<<(unsigned)((n + 255) / 256), 256>>>(pts, tmp, (int)logn);
  ZKR_HIP_CHECK(hipGetLastError());
  for (unsigned s = 0; s < logn; s++) {
    const uint32_t half = 1u << s;
    group_butterfly_kernel<C><<<(half_n + GROUP_THREADS - 1) / GROUP_THREADS, GROUP_THREADS>>>(tmp, (uint32_t)n, half, (const uint32_t *)tw, half_n / half, (W *)ztmp);
    ZKR_HIP_CHECK(hipGetLastError());
  }
  ZKR_HIP_CHECK(hipMemcpyAsync(pts, tmp, n * sizeof(Affine<W>), hipMemcpyDeviceToDevice, nullptr));
  if (inverse) {
    const Fr ninv = from_mont(inv(fr_small(n)));
    ZKR_HIP_CHECK(hipMemcpyAsync(tw + half_n, &ninv, sizeof(Fr), hipMemcpyHostToDevice, nullptr));
    ZKR_HIP_CHECK(hipStreamSynchronize(nullptr));  // `ninv` leaves the stack
    if (int rc = scale_each_launch<C>(pts, n, tw + half_n, 0, ztmp)) return rc;
  }
  return 0;
}

int sync_or_fail(const char *what) {
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("%s failed: %s", what, hipGetErrorString(e)); return ZKR_ERR_HIP; }
  return 0;
}

template <class C>
int scale_each_hook(void *points_mont, const void *scalars_std, size_t n, int device) {
  using W = typename C::W;
  DevBuf pts, sc, ztmp;
  int rc;
  if ((rc = pts.alloc(n * sizeof(Affine<W>))) || (rc = sc.alloc(n * 32)) || (rc = ztmp.alloc(2 * n * sizeof(W)))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(pts.p, points_mont, n * sizeof(Affine<W>), hipMemcpyHostToDevice));
  ZKR_HIP_CHECK(hipMemcpy(sc.p, scalars_std, n * 32, hipMemcpyHostToDevice));
  if ((rc = scale_each_launch<C>(pts.as<Affine<W>>(), n, sc.as<Fr>(), 1, ztmp.p)) || (rc = sync_or_fail("scaling the points"))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(points_mont, pts.p, n * sizeof(Affine<W>), hipMemcpyDeviceToHost));
  return 0;
}
template <class C>
int group_ntt_hook(void *points_mont, unsigned logn, bool inverse) {
  using W = typename C::W;
  const size_t n = (size_t)1 << logn;
  DevBuf pts, tmp, tw, ztmp;
  int rc;
  if ((rc = pts.alloc(n * sizeof(Affine<W>))) || (rc = tmp.alloc(n * sizeof(Affine<W>))) || (rc = tw.alloc((n / 2 + 1) * 32)) || (rc = ztmp.alloc(2 * n * sizeof(W)))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(pts.p, points_mont, n * sizeof(Affine<W>), hipMemcpyHostToDevice));
  if ((rc = group_ntt_launch<C>(pts.as<Affine<W>>(), tmp.as<Affine<W>>(), logn, inverse, tw.as<Fr>(), ztmp.p)) || (rc = sync_or_fail("the NTT over points"))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(points_mont, pts.p, n * sizeof(Affine<W>), hipMemcpyDeviceToHost));
  return 0;
}

// ---------------------------------------------------------------- a transcript on the device
// The body (everything after the header) as Montgomery affine points; vector v starts at body + off[v] - PTAU_HEADER.
struct DevicePtau {
  PtauLayout l;
  DevBuf body;
  template <class T> T *vec(int v) const { return (T *)(body.as<unsigned char>() + l.off[v] - PTAU_HEADER); }
};
// Uploads a transcript whose header passed ptau_header_fault and checks, BEFORE any group arithmetic reads it, that every
// coordinate is canonical and every point finite and on its curve (step 2).  *fault_vector < 0: fine.
int ptau_upload(const void *ptau, const PtauLayout &l, DevicePtau &d, int *fault_vector, char *why, size_t why_len) {
  d.l = l;
  *fault_vector = -1;
  const size_t body = l.total - PTAU_HEADER, n_coords = body / 32;
  FaultCounter bad;
  int rc;
  if ((rc = d.body.alloc(body)) || (rc = bad.reset())) return rc;
  ZKR_HIP_CHECK(hipMemcpy(d.body.p, (const uint8_t *)ptau + PTAU_HEADER, body, hipMemcpyHostToDevice));
  ptau_coords_in_kernel<<<(unsigned)((n_coords + 255) / 256), 256>>>(d.body.as<Fq>(), n_coords, bad.dev());
  if ((rc = bad.read())) return rc;
  if (bad.count) {
    const size_t at = PTAU_HEADER + 32 * (size_t)bad.first;  // the first of them, which names the vector
    int v = 0;
    while (v + 1 < N_VECTORS && at >= l.off[v + 1]) v++;
    *fault_vector = v;
    snprintf(why, why_len, "%u coordinate(s) are not below q (first: in entry %zu of %s)", bad.count, (at - l.off[v]) / (vector_is_g2(v) ? 128 : 64), VECTOR_NAME[v]);
    return 0;
  }
  for (int v = 0; v < N_VECTORS; v++) {
    if ((rc = bad.reset())) return rc;
    if (vector_is_g2(v)) group_on_curve_launch<Fq2>(d.vec<void>(v), (uint32_t)l.count[v], false, bad.dev());
    else group_on_curve_launch<Fq>(d.vec<void>(v), (uint32_t)l.count[v], false, bad.dev());
    if ((rc = bad.read())) return rc;
    if (bad.count) {
      *fault_vector = v;
      snprintf(why, why_len, "%u point(s) of %s are at infinity or off the curve (first: entry %u)", bad.count, VECTOR_NAME[v], bad.first);
      return 0;
    }
  }
  return 0;
}
// the body back in standard form, behind a fresh header, as a malloc'ed transcript
int ptau_download(DevicePtau &d, void **out, size_t *out_len) {
  const size_t body = d.l.total - PTAU_HEADER, n_coords = body / 32;
  ptau_coords_out_kernel<<<(unsigned)((n_coords + 255) / 256), 256>>>(d.body.as<Fq>(), n_coords);
  ZKR_HIP_CHECK(hipGetLastError());
  uint8_t *o = (uint8_t *)malloc(d.l.total);
  if (!o) { set_error("out of memory"); return ZKR_ERR_ARG; }
  ptau_write_header(o, d.l);
  const hipError_t e = hipMemcpy(o + PTAU_HEADER, d.body.p, body, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { free(o); set_error("download of the transcript failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  *out = o;
  *out_len = d.l.total;
  return 0;
}

// ---------------------------------------------------------------- the record (ZKR_PTAU_RECORD_BYTES)
// tau1_before | tau1_after | alfa1_before | alfa1_after | beta1_before | beta1_after | tau2_after | beta2_after | R_tau | R_alfa | R_beta |
// z_tau | z_alfa | z_beta, with tau1 = tauG1[1], alfa1 = alfaTauG1[0], beta1 = betaTauG1[0], tau2 = tauG2[1], beta2 = betaG2
constexpr size_t PREC_BEFORE[3] = {0, 128, 256}, PREC_AFTER[3] = {64, 192, 320}, PREC_G2[3] = {384, 0, 512}, PREC_R[3] = {640, 704, 768}, PREC_Z[3] = {832, 864, 896};
const char *const SECRET_NAME[3] = {"tau", "alfa", "beta"};
static_assert(PREC_Z[2] + 32 == ZKR_PTAU_RECORD_BYTES, "record layout");

// c = H(tag, before, after, [the G2 image], R): the library's host MiMC sponge over a domain tag (1, 2, 3) and the coordinates
int ptau_challenge(const uint8_t *rec, int which, uint8_t c_out[32]) {
  uint8_t in[11 * 32] = {0};
  size_t n = 0;
  in[0] = (uint8_t)(which + 1);
  n += 32;
  memcpy(in + n, rec + PREC_BEFORE[which], 64); n += 64;
  memcpy(in + n, rec + PREC_AFTER[which], 64); n += 64;
  if (which != 1) { memcpy(in + n, rec + PREC_G2[which], 128); n += 128; }
  memcpy(in + n, rec + PREC_R[which], 64); n += 64;
  return zkr_mimcsponge_multihash(in, n / 32, c_out);
}

struct ParsedPtauRecord {
  G1Affine before[3], after[3], r[3];
  G2Affine g2[3];  // [1] unused
};
// everything zkr_ptau_record_check states about ONE record; `why` (a buffer) names what failed
bool ptau_record_valid(const uint8_t *rec, ParsedPtauRecord &p, char *why, size_t why_len) {
  for (int k = 0; k < 3; k++) {
    const char *nm = SECRET_NAME[k];
    if (!read_g1_std(rec + PREC_BEFORE[k], p.before[k]) || !read_g1_std(rec + PREC_AFTER[k], p.after[k]) || !read_g1_std(rec + PREC_R[k], p.r[k])) {
      snprintf(why, why_len, "a G1 member of the %s proof is at infinity, out of range or off the curve", nm);
      return false;
    }
    if (k != 1 && !read_g2_std(rec + PREC_G2[k], p.g2[k])) { snprintf(why, why_len, "%s2_after is not a member of G2", nm); return false; }
    if (memcmp(rec + PREC_BEFORE[k], rec + PREC_AFTER[k], 64) == 0) { snprintf(why, why_len, "%s did not move", nm); return false; }
    if (!lt_words(rec + PREC_Z[k], FrParams::P)) { snprintf(why, why_len, "z_%s is not below r", nm); return false; }
    uint8_t c[32];
    if (ptau_challenge(rec, k, c)) { snprintf(why, why_len, "challenge hash failed"); return false; }
    if (!schnorr_verify(p.before[k], p.after[k], p.r[k], rec + PREC_Z[k], c)) { snprintf(why, why_len, "the proof of knowledge of %s does not verify", nm); return false; }
    if (k != 1 && !pairings_equal(p.after[k], g2_generator(), g1_generator(), p.g2[k])) {
      snprintf(why, why_len, "%s1_after and %s2_after are not the same multiple of the generators", nm, nm);
      return false;
    }
  }
  return true;
}
// a chain of records: each valid, the first starting at the generator, each next one where the previous ended
bool ptau_records_valid(const uint8_t *records, size_t n, char *why, size_t why_len) {
  uint8_t gen[64];
  store_g1_std(gen, g1_generator());
  for (size_t j = 0; j < n; j++) {
    const uint8_t *rec = records + j * ZKR_PTAU_RECORD_BYTES;
    ParsedPtauRecord p;
    char one[160];
    if (!ptau_record_valid(rec, p, one, sizeof(one))) { snprintf(why, why_len, "record %zu: %s", j, one); return false; }
    for (int k = 0; k < 3; k++) {
      const uint8_t *want = j == 0 ? gen : rec - ZKR_PTAU_RECORD_BYTES + PREC_AFTER[k];
      if (memcmp(rec + PREC_BEFORE[k], want, 64) != 0) {
        snprintf(why, why_len, j == 0 ? "record %zu: the chain does not start at the generator (%s1_before)" : "record %zu: the chain is broken (%s1_before is not the previous record's %s1_after)", j,
                 SECRET_NAME[k], SECRET_NAME[k]);
        return false;
      }
    }
  }
  return true;
}

// ---------------------------------------------------------------- verification of a transcript (steps 1-5 of zkr_ptau_verify)
struct PtauVerdict {
  uint64_t step = 0, vector = 0;  // the first failed step (0: none) and the vector it was found in
  char why[240] = "";
};
// sum_i sc[i] pts[i] by the library's MSM path (host buffers, Montgomery affine points); *inf: the sum is the point at infinity
int msm_g1_host(const uint8_t *pts, const uint8_t *sc, size_t n, int device, G1Affine &out, bool &inf) {
  uint8_t o[64];
  int is_inf = 0;
  if (int rc = zkr_msm_g1(pts, sc, n, o, &is_inf, device)) return rc;
  inf = is_inf != 0;
  if (!inf) out = G1Affine{to_mont(load_fp<FqParams>(o)), to_mont(load_fp<FqParams>(o + 32))};
  return 0;
}
int msm_g2_host(const uint8_t *pts, const uint8_t *sc, size_t n, int device, G2Affine &out, bool &inf) {
  uint8_t o[128];
  int is_inf = 0;
  if (int rc = zkr_msm_g2(pts, sc, n, o, &is_inf, device)) return rc;
  inf = is_inf != 0;
  if (!inf) out = G2Affine{Fq2{to_mont(load_fp<FqParams>(o)), to_mont(load_fp<FqParams>(o + 32))}, Fq2{to_mont(load_fp<FqParams>(o + 64)), to_mont(load_fp<FqParams>(o + 96))}};
  return 0;
}

// Steps 2-5 on a transcript whose header passed (step 1); `d`: its device form, left in place for the caller.  A status below
// zero only for a HIP failure; a bad transcript is v.step != 0 with a message.
int ptau_check(const void *ptau, const PtauLayout &l, int device, DevicePtau &d, PtauVerdict &v) {
  auto fail = [&](uint64_t step, uint64_t vector, const char *what) {
    v.step = step; v.vector = vector;
    snprintf(v.why, sizeof(v.why), "step %llu failed (%s): %s", (unsigned long long)step, VECTOR_NAME[vector], what);
    return 0;
  };
  int rc, fault = -1;
  char why[160];
  // 2. canonical coordinates, finite points on their curves -- before any group arithmetic reads them
  if ((rc = ptau_upload(ptau, l, d, &fault, why, sizeof(why)))) return rc;
  if (fault >= 0) return fail(2, (uint64_t)fault, why);
  const size_t M = l.M;
  // 3. every G2 point has order r: [r] Q == O, point by point
  {
    uint32_t naf[16];
    U256 r;
    memcpy(r.v, FrParams::P, 32);
    const int top = naf_of(r, naf, naf + 8);
    DevBuf dn;
    FaultCounter bad;
    if ((rc = dn.alloc(sizeof(naf)))) return rc;
    ZKR_HIP_CHECK(hipMemcpy(dn.p, naf, sizeof(naf), hipMemcpyHostToDevice));
    for (int vec : {V_TAU2, V_BETA2}) {
      const uint32_t n = (uint32_t)l.count[vec];
      if ((rc = bad.reset())) return rc;
      group_order_check_kernel<G2C><<<(n + GROUP_THREADS - 1) / GROUP_THREADS, GROUP_THREADS>>>(d.vec<G2Affine>(vec), n, dn.as<uint32_t>(), top, bad.dev());
      if ((rc = bad.read())) return rc;
      if (bad.count) {
        snprintf(why, sizeof(why), "%u point(s) are on the twist but outside the order-r subgroup G2 (first: entry %u)", bad.count, bad.first);
        return fail(3, (uint64_t)vec, why);
      }
    }
  }
  // 4. the vectors start at the generators
  {
    uint8_t g1[64], g2[128];
    store_g1_std(g1, g1_generator());
    store_g2_std(g2, g2_generator());
    if (memcmp((const uint8_t *)ptau + l.off[V_TAU1], g1, 64) != 0) return fail(4, V_TAU1, "tauG1[0] is not the generator of G1");
    if (memcmp((const uint8_t *)ptau + l.off[V_TAU2], g2, 128) != 0) return fail(4, V_TAU2, "tauG2[0] is not the generator of G2");
  }
  // 5. every vector is the geometric progression it claims to be: random 128-bit combinations (2^-128 per wrong entry), the sums
  //    by the library's MSM path, a few pairings on the host
  std::vector<uint8_t> h[N_VECTORS];
  for (int vec = 0; vec < N_VECTORS; vec++) {
    h[vec].resize(l.count[vec] * (vector_is_g2(vec) ? 128 : 64));
    ZKR_HIP_CHECK(hipMemcpy(h[vec].data(), d.vec<unsigned char>(vec), h[vec].size(), hipMemcpyDeviceToHost));
  }
  std::vector<uint8_t> rho, sigma;
  if ((rc = random_128(rho, 2 * M - 1)) || (rc = random_128(sigma, M))) return rc;
  const G1Affine G1 = g1_generator(), tau1 = load_g1(&h[V_TAU1][64]), alfa1 = load_g1(h[V_ALFA1].data()), beta1 = load_g1(h[V_BETA1].data());
  const G2Affine G2 = g2_generator(), tau2 = load_g2(&h[V_TAU2][128]), beta2 = load_g2(h[V_BETA2].data());
  bool i0 = false, i1 = false;
  {  // e(sum rho_i tauG1[i + 1], G2) == e(sum rho_i tauG1[i], tauG2[1])
    G1Affine hi, lo;
    if ((rc = msm_g1_host(&h[V_TAU1][64], rho.data(), 2 * M - 1, device, hi, i1)) || (rc = msm_g1_host(h[V_TAU1].data(), rho.data(), 2 * M - 1, device, lo, i0))) return rc;
    if (i0 || i1 || !pairings_equal(hi, G2, lo, tau2)) return fail(5, V_TAU1, "tauG1 is not the sequence of powers tauG2[1] stands for");
  }
  G2Affine T;  // sum_{i < M} sigma_i tauG2[i]
  {  // e(tauG1[1], S0) == e(G1, S1), S0 = sum_{i < M - 1} sigma_i tauG2[i], S1 the same over tauG2[i + 1]
    G2Affine s0, s1;
    if ((rc = msm_g2_host(h[V_TAU2].data(), sigma.data(), M - 1, device, s0, i0)) || (rc = msm_g2_host(&h[V_TAU2][128], sigma.data(), M - 1, device, s1, i1))) return rc;
    if (i0 || i1 || !pairings_equal(tau1, s0, G1, s1)) return fail(5, V_TAU2, "tauG2 is not the sequence of powers tauG1[1] stands for");
    const G2XYZZ t = add_full(to_xyzz(s0), scalar_mul(to_xyzz(load_g2(&h[V_TAU2][128 * (M - 1)])), load_u256(&sigma[32 * (M - 1)])));
    if (t.is_inf()) return fail(5, V_TAU2, "a random combination of tauG2 vanished");
    T = to_affine(t);
  }
  for (int vec : {V_ALFA1, V_BETA1}) {  // e(sum sigma_i xTauG1[i], G2) == e(xTauG1[0], T)
    G1Affine sum;
    if ((rc = msm_g1_host(h[vec].data(), sigma.data(), M, device, sum, i0))) return rc;
    if (i0 || !pairings_equal(sum, G2, vec == V_ALFA1 ? alfa1 : beta1, T)) return fail(5, (uint64_t)vec, "the vector is not its first entry times the powers of tau");
  }
  if (!pairings_equal(beta1, G2, G1, beta2)) return fail(5, V_BETA2, "betaG2 and betaTauG1[0] are not the same multiple of the generators");
  return 0;
}

// ---------------------------------------------------------------- sparse combinations: the host's plan
// One thread sums one task, so a task is bounded in the WORK it holds, not only in its terms: a term of magnitude one is an
// addition, any other a ladder as long as its magnitude.  Signal 0 of the tx circuit sits in tens of thousands of rows, many of
// them with full-width coefficients (the MiMC round constants); cut by terms alone, its tasks ran 256 ladders one after the other
// and the launch waited half a second for a handful of threads.  A column that does not fit one task becomes partial sums, and
// the partial sums are summed by further launches of the same kernel (row[e] then points into the output array itself) until one
// task per column is left.
constexpr uint32_t COMBINE_TASK_TERMS = 256;  // most terms of a task
constexpr uint32_t COMBINE_TASK_STEPS = 512;  // most ladder steps of a task (two full-width coefficients)
struct CombineLevel {
  std::vector<uint32_t> tb{0}, dst, row, meta;  // task t: terms [tb[t], tb[t + 1]) -> out[dst[t]]
};
struct CombinePlan {
  std::vector<CombineLevel> levels;  // levels[0] over the source points, the others over the partial sums of the one before
  std::vector<uint32_t> mag;         // 8 words per term of levels[0]
  size_t n_out = 0;                  // signals + partial sums
};
int bit_length(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--)
    if (w[i]) return 32 * i + 32 - __builtin_clz(w[i]);
  return 0;
}
// the columns of `nsrc` matrices side by side (source k's rows shifted by row_off[k]): out[s] = sum_k sum_e coef x pts[row + row_off[k]]
void combine_plan(uint32_t n, const QapColumns *const *src, const uint32_t *row_off, int nsrc, CombinePlan &pl) {
  uint32_t next = n;  // the next partial sum's index in the output array
  std::vector<std::pair<uint32_t, std::vector<uint32_t>>> open;  // columns that are partial sums so far: (signal, their indices)
  pl.levels.emplace_back();
  {
    CombineLevel &l = pl.levels[0];
    std::vector<uint32_t> order, sorted_row, sorted_meta, sorted_mag;
    for (uint32_t s = 0; s < n; s++) {
      std::vector<uint32_t> parts;
      uint32_t terms = 0, steps = 0;
      auto close_task = [&](uint32_t to) {
        // The ladders first, longest first: a wavefront's 64 tasks then run their ladders in the same iterations of the term loop.
        // In column order each lane met its ladders at iterations of its own and the wave ran them one lane after the other.
        const size_t b = l.tb.back(), e = l.row.size();
        order.resize(e - b);
        for (size_t i = 0; i < e - b; i++) order[i] = (uint32_t)(b + i);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return (l.meta[x] & 0x1ffu) > (l.meta[y] & 0x1ffu); });
        if (!std::is_sorted(order.begin(), order.end())) {
          sorted_row.clear(); sorted_meta.clear(); sorted_mag.clear();
          for (uint32_t i : order) {
            sorted_row.push_back(l.row[i]);
            sorted_meta.push_back(l.meta[i]);
            sorted_mag.insert(sorted_mag.end(), pl.mag.begin() + 8 * (size_t)i, pl.mag.begin() + 8 * (size_t)i + 8);
          }
          std::copy(sorted_row.begin(), sorted_row.end(), l.row.begin() + b);
          std::copy(sorted_meta.begin(), sorted_meta.end(), l.meta.begin() + b);
          std::copy(sorted_mag.begin(), sorted_mag.end(), pl.mag.begin() + 8 * b);
        }
        l.tb.push_back((uint32_t)l.row.size());
        l.dst.push_back(to);
        terms = steps = 0;
      };
      for (int k = 0; k < nsrc; k++)
        for (uint32_t e = src[k]->colptr[s]; e < src[k]->colptr[s + 1]; e++) {
          uint32_t c[8], neg[8];
          memcpy(c, &src[k]->coef[32 * (size_t)e], 32);
          uint64_t borrow = 0;
          for (int i = 0; i < 8; i++) {  // r - c
            const uint64_t dlt = (uint64_t)FrParams::P[i] - c[i] - borrow;
            neg[i] = (uint32_t)dlt;
            borrow = (dlt >> 32) & 1;
          }
          const int bc = bit_length(c), bn = bit_length(neg);
          const bool minus = bc != 0 && bn < bc;
          const uint32_t bits = (uint32_t)(minus ? bn : bc);
          if (terms && (terms + 1 > COMBINE_TASK_TERMS || steps + bits > COMBINE_TASK_STEPS)) {
            parts.push_back(next);
            close_task(next++);
          }
          l.row.push_back(src[k]->row[e] + row_off[k]);
          l.meta.push_back(bits | (minus ? 0x80000000u : 0u));
          pl.mag.insert(pl.mag.end(), minus ? neg : c, (minus ? neg : c) + 8);
          terms++;
          steps += bits;
        }
      if (parts.empty()) { close_task(s); continue; }  // the whole column (or none of it: infinity) in one task
      parts.push_back(next);
      close_task(next++);
      open.emplace_back(s, std::move(parts));
    }
  }
  while (!open.empty()) {
    pl.levels.emplace_back();
    CombineLevel &l = pl.levels.back();
    std::vector<std::pair<uint32_t, std::vector<uint32_t>>> still;
    for (auto &col : open) {
      const std::vector<uint32_t> &parts = col.second;
      std::vector<uint32_t> fewer;
      for (size_t b = 0; b < parts.size(); b += COMBINE_TASK_TERMS) {
        const size_t e = b + COMBINE_TASK_TERMS < parts.size() ? b + COMBINE_TASK_TERMS : parts.size();
        l.row.insert(l.row.end(), parts.begin() + b, parts.begin() + e);
        l.meta.insert(l.meta.end(), e - b, 1u);
        l.tb.push_back((uint32_t)l.row.size());
        if (parts.size() <= COMBINE_TASK_TERMS) l.dst.push_back(col.first);
        else { l.dst.push_back(next); fewer.push_back(next++); }
      }
      if (!fewer.empty()) still.emplace_back(col.first, std::move(fewer));
    }
    open.swap(still);
  }
  pl.n_out = next;
}
struct DeviceCombinePlan {
  struct Level {
    DevBuf tb, dst, row, meta;
    uint32_t n_tasks = 0;
  };
  std::vector<Level> levels;
  DevBuf mag;
  size_t n_out = 0;
  int upload(const CombinePlan &pl) {
    auto up = [](DevBuf &b, const std::vector<uint32_t> &v) -> int {
      if (int rc = b.alloc(v.size() * 4)) return rc;
      if (!v.empty()) ZKR_HIP_CHECK(hipMemcpy(b.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
      return 0;
    };
    int rc;
    if ((rc = up(mag, pl.mag))) return rc;
    levels = std::vector<Level>(pl.levels.size());
    for (size_t k = 0; k < pl.levels.size(); k++) {
      const CombineLevel &h = pl.levels[k];
      Level &l = levels[k];
      if ((rc = up(l.tb, h.tb)) || (rc = up(l.dst, h.dst)) || (rc = up(l.row, h.row)) || (rc = up(l.meta, h.meta))) return rc;
      l.n_tasks = (uint32_t)h.dst.size();
    }
    n_out = pl.n_out;
    return 0;
  }
};
// out (n_out points, a fresh allocation) = the plan's combinations of `pts`
template <class C>
int combine_run(const DeviceCombinePlan &dp, const Affine<typename C::W> *pts, void *ztmp, DevBuf &out) {
  using W = typename C::W;
  DevBuf o;
  if (int rc = o.alloc(dp.n_out * sizeof(Affine<W>))) return rc;
  for (size_t k = 0; k < dp.levels.size(); k++) {
    const DeviceCombinePlan::Level &l = dp.levels[k];
    if (!l.n_tasks) continue;
    group_combine_kernel<C><<<(l.n_tasks + GROUP_THREADS - 1) / GROUP_THREADS, GROUP_THREADS>>>(o.as<Affine<W>>(), (W *)ztmp, dp.n_out, l.n_tasks, l.tb.as<uint32_t>(), l.dst.as<uint32_t>(),
                                                                                          l.row.as<uint32_t>(), l.meta.as<uint32_t>(), dp.mag.as<uint32_t>(),
                                                                                          k == 0 ? pts : o.as<Affine<W>>());
    ZKR_HIP_CHECK(hipGetLastError());
  }
  out = std::move(o);
  return 0;
}

// everything that reveals tau, alfa or beta: wiped however zkr_ptau_contribute is left
struct PtauSecrets {
  U256 s[3], nonce[3];
  Fr sm[3];
  ResponseScratch resp;  // wipes itself
  DevBuf powers;  // tau^i (2 M) | alfa tau^i (M) | beta tau^i (M): Montgomery while they are built, then standard form
  DevBuf ztmp;    // the ZZ, ZZZ of the ladders' unnormalised results: functions of the secret scalars
  size_t powers_bytes = 0, ztmp_bytes = 0;
  ~PtauSecrets() {
    if (powers.p) (void)hipMemset(powers.p, 0, powers_bytes);
    if (ztmp.p) (void)hipMemset(ztmp.p, 0, ztmp_bytes);
    if (powers.p || ztmp.p) (void)hipDeviceSynchronize();
    explicit_bzero(s, sizeof(s)); explicit_bzero(nonce, sizeof(nonce)); explicit_bzero(sm, sizeof(sm));
  }
};

}  // namespace

int ptau_key_tables(const void *ptau, size_t len, int device, uint32_t m, uint32_t n, const QapColumns cols[3], DevBuf d_tbl[N_TABLES], uint8_t consts448[448]) {
  PtauLayout l;
  if (const char *f = ptau_header_fault(ptau, len, l)) { set_error("zkr_setup_r1cs_ptau: %s", f); return ZKR_ERR_ARG; }
  if (m > l.M) { set_error("zkr_setup_r1cs_ptau: the circuit's domain is %u; a transcript of power %u serves domains up to 2^%u", m, l.power, l.power); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  DevicePtau d;
  PtauVerdict v;
  int rc;
  if ((rc = ptau_check(ptau, l, device, d, v))) return rc;
  if (v.step) { set_error("zkr_setup_r1cs_ptau: the transcript does not verify: %s", v.why); return ZKR_ERR_BAD_KEY; }
  const unsigned logm = domain_log2(m);

  // the plans of the three combinations: A over Lag1; B over Lag1 and Lag2; K over [Lag1 | LagAlfa | LagBeta] with A's rows in
  // the beta slice, B's in the alfa slice, C's in the first
  CombinePlan pa, pb, pk;
  {
    const QapColumns *sa[1] = {&cols[0]}, *sb[1] = {&cols[1]}, *sk[3] = {&cols[0], &cols[1], &cols[2]};
    const uint32_t zero[1] = {0}, offk[3] = {2 * m, m, 0};
    combine_plan(n, sa, zero, 1, pa);
    combine_plan(n, sb, zero, 1, pb);
    combine_plan(n, sk, offk, 3, pk);
  }
  size_t n_max = pa.n_out > pb.n_out ? pa.n_out : pb.n_out;
  n_max = n_max > pk.n_out ? n_max : pk.n_out;
  n_max = n_max > m ? n_max : m;

  // Lagrange-basis points of the first m powers: the inverse NTT over points
  DevBuf lag1, lag2, tmp, tw, ztmp;
  if ((rc = lag1.alloc(3 * (size_t)m * sizeof(G1Affine))) || (rc = lag2.alloc((size_t)m * sizeof(G2Affine))) || (rc = tmp.alloc((size_t)m * sizeof(G2Affine))) ||
      (rc = tw.alloc(((size_t)m / 2 + 1) * sizeof(Fr))) || (rc = ztmp.alloc(2 * n_max * sizeof(Fq2))))
    return rc;
  const int slice_src[3] = {V_TAU1, V_ALFA1, V_BETA1};
  for (int k = 0; k < 3; k++) {
    ZKR_HIP_CHECK(hipMemcpy(lag1.as<G1Affine>() + (size_t)k * m, d.vec<G1Affine>(slice_src[k]), (size_t)m * sizeof(G1Affine), hipMemcpyDeviceToDevice));
    if ((rc = group_ntt_launch<G1C>(lag1.as<G1Affine>() + (size_t)k * m, tmp.as<G1Affine>(), logm, true, tw.as<Fr>(), ztmp.p))) return rc;
  }
  ZKR_HIP_CHECK(hipMemcpy(lag2.p, d.vec<G2Affine>(V_TAU2), (size_t)m * sizeof(G2Affine), hipMemcpyDeviceToDevice));
  if ((rc = group_ntt_launch<G2C>(lag2.as<G2Affine>(), tmp.as<G2Affine>(), logm, true, tw.as<Fr>(), ztmp.p))) return rc;

  DevBuf out[N_TABLES];  // handed over when all five are complete
  {
    DeviceCombinePlan dp;
    if ((rc = dp.upload(pa)) || (rc = combine_run<G1C>(dp, lag1.as<G1Affine>(), ztmp.p, out[T_A])) || (rc = sync_or_fail("the A points"))) return rc;
  }
  {
    DeviceCombinePlan dp;
    if ((rc = dp.upload(pb)) || (rc = combine_run<G1C>(dp, lag1.as<G1Affine>(), ztmp.p, out[T_B1])) || (rc = combine_run<G2C>(dp, lag2.as<G2Affine>(), ztmp.p, out[T_B2])) ||
        (rc = sync_or_fail("the B points")))
      return rc;
  }
  {
    DeviceCombinePlan dp;
    if ((rc = dp.upload(pk)) || (rc = combine_run<G1C>(dp, lag1.as<G1Affine>(), ztmp.p, out[T_C])) || (rc = sync_or_fail("the C and IC points"))) return rc;
  }
  // hExps[i] = (tau^(i + m) - tau^i) G1 = tau^i Z(tau) G1
  {
    DevBuf hx;
    if ((rc = hx.alloc((size_t)m * sizeof(G1Affine)))) return rc;
    group_diff_kernel<G1C><<<(m + GROUP_THREADS - 1) / GROUP_THREADS, GROUP_THREADS>>>(hx.as<G1Affine>(), d.vec<G1Affine>(V_TAU1) + m, d.vec<G1Affine>(V_TAU1), m, ztmp.as<Fq>());
    ZKR_HIP_CHECK(hipGetLastError());
    if ((rc = sync_or_fail("the H points"))) return rc;
    out[T_H] = std::move(hx);
  }
  // vk_alfa_1, vk_beta_1, vk_delta_1 | vk_beta_2, vk_delta_2 with delta = 1
  ZKR_HIP_CHECK(hipMemcpy(consts448, d.vec<unsigned char>(V_ALFA1), 64, hipMemcpyDeviceToHost));
  ZKR_HIP_CHECK(hipMemcpy(consts448 + 64, d.vec<unsigned char>(V_BETA1), 64, hipMemcpyDeviceToHost));
  ZKR_HIP_CHECK(hipMemcpy(consts448 + 192, d.vec<unsigned char>(V_BETA2), 128, hipMemcpyDeviceToHost));
  store_g1_mont(consts448 + 128, g1_generator());
  store_g2_mont(consts448 + 320, g2_generator());
  for (int t = 0; t < N_TABLES; t++) d_tbl[t] = std::move(out[t]);
  return 0;
}

// the same launches for the side tables a key derives from its own points (zkr_internal.hpp)
int g1_scale_each(G1Affine *pts, size_t n, const Fr *d_scalars, uint32_t sc_stride, void *ztmp) { return scale_each_launch<G1C>(pts, n, d_scalars, sc_stride, ztmp); }
int g1_group_ntt(G1Affine *pts, G1Affine *tmp, unsigned logn, bool inverse, Fr *tw, void *ztmp) { return group_ntt_launch<G1C>(pts, tmp, logn, inverse, tw, ztmp); }
int g1_combine_columns(uint32_t n, const QapColumns &cols, const G1Affine *pts, DevBuf &out) {
  CombinePlan pl;
  const QapColumns *src[1] = {&cols};
  const uint32_t zero[1] = {0};
  combine_plan(n, src, zero, 1, pl);
  DeviceCombinePlan dp;
  DevBuf ztmp;
  int rc;
  if ((rc = dp.upload(pl)) || (rc = ztmp.alloc(2 * pl.n_out * sizeof(Fq))) || (rc = combine_run<G1C>(dp, pts, ztmp.p, out))) return rc;
  if ((rc = sync_or_fail("combining the points"))) out.reset();
  return rc;
}

const char *ptau_shape_fault(const void *ptau, size_t len, unsigned *power) {
  PtauLayout l;
  const char *f = ptau_header_fault(ptau, len, l);
  if (!f && power) *power = l.power;
  return f;
}

// zkr_ptau_verify (include/zkr.h has the steps); keep: where the device form of a transcript that verified goes
int ptau_verify_keep(const void *ptau, size_t len, const uint8_t *records, size_t n_records, int device, int *valid, uint64_t report[2], PtauOnDevice *keep) {
  if (!ptau || !valid || (n_records && !records)) { set_error("null argument"); return ZKR_ERR_ARG; }
  *valid = 0;
  uint64_t rep_local[2];
  uint64_t *rep = report ? report : rep_local;
  rep[0] = rep[1] = 0;
  PtauLayout l;
  if (const char *f = ptau_header_fault(ptau, len, l)) { rep[0] = 1; set_error("ptau verify: step 1 failed: %s", f); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  DevicePtau d;
  PtauVerdict v;
  if (int rc = ptau_check(ptau, l, device, d, v)) return rc;
  if (v.step) {
    rep[0] = v.step; rep[1] = v.vector;
    set_error("ptau verify: %s", v.why);
    return 0;
  }
  // 6. the records verify, chain from the generators, and end at THIS transcript
  auto fail6 = [&](uint64_t vector, const char *what) {
    rep[0] = 6; rep[1] = vector;
    set_error("ptau verify: step 6 failed: %s", what);
    return 0;
  };
  char why[256];
  if (!ptau_records_valid(records, n_records, why, sizeof(why))) return fail6(0, why);
  const uint8_t *b = (const uint8_t *)ptau;
  uint8_t g1[64], g2[128];
  store_g1_std(g1, g1_generator());
  store_g2_std(g2, g2_generator());
  const uint8_t *last = n_records ? records + (n_records - 1) * ZKR_PTAU_RECORD_BYTES : nullptr;
  const struct { int vec; size_t at; const uint8_t *want; size_t bytes; } ends[5] = {
      {V_TAU1, l.off[V_TAU1] + 64, last ? last + PREC_AFTER[0] : g1, 64},   {V_ALFA1, l.off[V_ALFA1], last ? last + PREC_AFTER[1] : g1, 64},
      {V_BETA1, l.off[V_BETA1], last ? last + PREC_AFTER[2] : g1, 64},      {V_TAU2, l.off[V_TAU2] + 128, last ? last + PREC_G2[0] : g2, 128},
      {V_BETA2, l.off[V_BETA2], last ? last + PREC_G2[2] : g2, 128}};
  for (const auto &e : ends)
    if (memcmp(b + e.at, e.want, e.bytes) != 0) {
      snprintf(why, sizeof(why), last ? "the last record does not end at this transcript's %s" : "no records, but %s is not the all-generators transcript's", VECTOR_NAME[e.vec]);
      return fail6((uint64_t)e.vec, why);
    }
  *valid = 1;
  if (keep) {
    keep->power = l.power; keep->M = l.M;
    keep->off_tau1 = l.off[V_TAU1]; keep->off_tau2 = l.off[V_TAU2]; keep->off_alfa1 = l.off[V_ALFA1]; keep->off_beta1 = l.off[V_BETA1]; keep->off_beta2 = l.off[V_BETA2];
    keep->tau1 = d.vec<G1Affine>(V_TAU1); keep->alfa1 = d.vec<G1Affine>(V_ALFA1); keep->beta1 = d.vec<G1Affine>(V_BETA1);
    keep->tau2 = d.vec<G2Affine>(V_TAU2); keep->beta2 = d.vec<G2Affine>(V_BETA2);
    keep->body = std::move(d.body);
  }
  return 0;
}

}  // namespace zkr

using namespace zkr;

extern "C" {

int zkr_points_scale_each(void *points_mont, const void *scalars_std, size_t n, int g2, int device) {
  if (!points_mont || !scalars_std) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (n > 0xffffffffu) { set_error("zkr_points_scale_each: at most 2^32 - 1 points"); return ZKR_ERR_ARG; }
  for (size_t i = 0; i < n; i++)
    if (!lt_words((const uint8_t *)scalars_std + 32 * i, FrParams::P)) { set_error("zkr_points_scale_each: scalar %zu is not below r", i); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  if (!n) return 0;
  return g2 ? scale_each_hook<G2C>(points_mont, scalars_std, n, device) : scale_each_hook<G1C>(points_mont, scalars_std, n, device);
}

int zkr_group_ntt(void *points_mont, unsigned logn, int inverse, int g2, int device) {
  if (!points_mont || logn < 1 || logn > 25) { set_error("bad argument (logn 1..25)"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  return g2 ? group_ntt_hook<G2C>(points_mont, logn, inverse != 0) : group_ntt_hook<G1C>(points_mont, logn, inverse != 0);
}

int zkr_ptau_new(unsigned power, void **ptau_out, size_t *ptau_len) {
  if (!ptau_out || !ptau_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (power < 1 || power > PTAU_MAX_POWER) { set_error("zkr_ptau_new: power %u outside 1..%u", power, PTAU_MAX_POWER); return ZKR_ERR_ARG; }
  const PtauLayout l = ptau_layout(power);
  uint8_t *o = (uint8_t *)malloc(l.total);
  if (!o) { set_error("out of memory"); return ZKR_ERR_ARG; }
  ptau_write_header(o, l);
  uint8_t g1[64], g2[128];
  store_g1_std(g1, g1_generator());
  store_g2_std(g2, g2_generator());
  for (int v = 0; v < N_VECTORS; v++)
    for (size_t i = 0; i < l.count[v]; i++) {
      if (vector_is_g2(v)) memcpy(o + l.off[v] + 128 * i, g2, 128);
      else memcpy(o + l.off[v] + 64 * i, g1, 64);
    }
  *ptau_out = o;
  *ptau_len = l.total;
  return 0;
}

int zkr_ptau_record_check(const uint8_t *records, size_t n_records, int *valid) {
  if (!records || !valid) { set_error("null argument"); return ZKR_ERR_ARG; }
  char why[256];
  *valid = ptau_records_valid(records, n_records, why, sizeof(why)) ? 1 : 0;
  if (!*valid) set_error("ptau record check: %s", why);
  return 0;
}

int zkr_ptau_verify(const void *ptau, size_t len, const uint8_t *records, size_t n_records, int device, int *valid, uint64_t report[2]) {
  return ptau_verify_keep(ptau, len, records, n_records, device, valid, report, nullptr);
}

int zkr_ptau_contribute(const void *ptau, size_t len, const uint8_t *secrets96, int device, void **ptau_out, size_t *out_len, uint8_t record_out[ZKR_PTAU_RECORD_BYTES]) {
  if (!ptau || !ptau_out || !out_len || !record_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  PtauLayout l;
  if (const char *f = ptau_header_fault(ptau, len, l)) { set_error("zkr_ptau_contribute: %s", f); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  PtauSecrets s;
  int rc;
  for (int k = 0; k < 3; k++) {
    if (secrets96) {
      if (!valid_secret(secrets96 + 32 * k)) { set_error("zkr_ptau_contribute: %s must satisfy 1 < s < r", SECRET_NAME[k]); return ZKR_ERR_ARG; }
      memcpy(s.s[k].v, secrets96 + 32 * k, 32);
    } else if ((rc = draw_secret(s.s[k]))) return rc;
    if ((rc = draw_secret(s.nonce[k]))) return rc;
    memcpy(s.sm[k].v, s.s[k].v, 32);
    s.sm[k] = to_mont(s.sm[k]);
  }
  ZKR_HIP_CHECK(hipSetDevice(device));
  DevicePtau d;
  int fault = -1;
  char why[160];
  if ((rc = ptau_upload(ptau, l, d, &fault, why, sizeof(why)))) return rc;
  if (fault >= 0) { set_error("zkr_ptau_contribute: %s", why); return ZKR_ERR_ARG; }

  // the powers: T[i] = tau^i (i < 2 M), alfa T[i], beta T[i] (i < M), by the library's twiddle-table kernel; then standard form
  const size_t M = l.M;
  s.powers_bytes = 4 * M * sizeof(Fr);
  s.ztmp_bytes = 2 * (2 * M) * sizeof(Fq);
  DevBuf &ztmp = s.ztmp;
  if ((rc = s.powers.alloc(s.powers_bytes)) || (rc = ztmp.alloc(s.ztmp_bytes))) return rc;  // 2 x 2 M Fq = 2 x M Fq2: the largest vector of either group
  Fr *T = s.powers.as<Fr>(), *Ta = T + 2 * M, *Tb = T + 3 * M;
  twiddle_table_kernel<<<(unsigned)((2 * M + 255) / 256), 256>>>(T, (uint32_t)(2 * M), s.sm[0]);
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpyAsync(Ta, T, M * sizeof(Fr), hipMemcpyDeviceToDevice, nullptr));
  ZKR_HIP_CHECK(hipMemcpyAsync(Tb, T, M * sizeof(Fr), hipMemcpyDeviceToDevice, nullptr));
  scale_kernel<<<(unsigned)((M + 255) / 256), 256>>>(Ta, M, s.sm[1]);
  scale_kernel<<<(unsigned)((M + 255) / 256), 256>>>(Tb, M, s.sm[2]);
  fr_to_std_kernel<<<(unsigned)((4 * M + 255) / 256), 256>>>(T, (uint32_t)(4 * M));
  ZKR_HIP_CHECK(hipGetLastError());
  if ((rc = scale_each_launch<G1C>(d.vec<G1Affine>(V_TAU1), 2 * M, T, 1, ztmp.p)) || (rc = scale_each_launch<G2C>(d.vec<G2Affine>(V_TAU2), M, T, 1, ztmp.p)) ||
      (rc = scale_each_launch<G1C>(d.vec<G1Affine>(V_ALFA1), M, Ta, 1, ztmp.p)) || (rc = scale_each_launch<G1C>(d.vec<G1Affine>(V_BETA1), M, Tb, 1, ztmp.p)) ||
      (rc = scale_each_launch<G2C>(d.vec<G2Affine>(V_BETA2), 1, Tb, 1, ztmp.p)) || (rc = sync_or_fail("scaling the transcript")))
    return rc;
  void *out = nullptr;
  size_t olen = 0;
  if ((rc = ptau_download(d, &out, &olen))) return rc;
  struct Owner {  // the new transcript goes unless it is handed over
    void *p;
    ~Owner() { free(p); }
  } owner{out};

  // the record (host; a few hundred group operations)
  const uint8_t *in_b = (const uint8_t *)ptau, *out_b = (const uint8_t *)out;
  const size_t at[3] = {l.off[V_TAU1] + 64, l.off[V_ALFA1], l.off[V_BETA1]};
  uint8_t rec[ZKR_PTAU_RECORD_BYTES];
  memcpy(rec + PREC_G2[0], out_b + l.off[V_TAU2] + 128, 128);
  memcpy(rec + PREC_G2[2], out_b + l.off[V_BETA2], 128);
  for (int k = 0; k < 3; k++) {
    memcpy(rec + PREC_BEFORE[k], in_b + at[k], 64);
    memcpy(rec + PREC_AFTER[k], out_b + at[k], 64);
    G1Affine before;
    if (!read_g1_std(rec + PREC_BEFORE[k], before)) { set_error("zkr_ptau_contribute: the transcript's %s1 is not a point of G1", SECRET_NAME[k]); return ZKR_ERR_ARG; }
    const G1XYZZ r_x = scalar_mul(to_xyzz(before), s.nonce[k]);
    if (r_x.is_inf()) { set_error("zkr_ptau_contribute: the transcript's %s1 is not a point of order r", SECRET_NAME[k]); return ZKR_ERR_ARG; }
    store_g1_std(rec + PREC_R[k], to_affine(r_x));
    uint8_t c[32];
    if ((rc = ptau_challenge(rec, k, c))) return rc;
    schnorr_response(s.nonce[k], c, s.sm[k], s.resp, rec + PREC_Z[k]);
  }
  memcpy(record_out, rec, ZKR_PTAU_RECORD_BYTES);
  *ptau_out = out;
  *out_len = olen;
  owner.p = nullptr;
  return 0;
}

}  // extern "C"
