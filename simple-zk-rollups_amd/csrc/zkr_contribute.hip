// zkr_contribute.hip -- a further party's delta contribution to a device key, with a record anybody can check.
//
// zkr_setup_r1cs is a one-party setup (as `snarkjs setup` in the reference's workflow, prover/package.json:34,37):
// whoever ran it could know delta, and delta forges proofs.  A contributor draws d and re-randomises delta without any of the
// toxic values:
//     delta1' = d delta1    delta2' = d delta2    C'[s] = d^-1 C[s]  (s > nPublic)    hExps'[i] = d^-1 hExps[i]
// which is exactly the key a setup with delta d would have produced.  This protects against the earlier DELTA holders only: the
// runner of a one-party setup also knows t, alfa and beta, which forge on their own -- a key that can guard deposits starts from
// a powers-of-tau transcript (zkr_ptau.hip, zkr_setup_r1cs_ptau) and takes its delta contributions after that.
//
// The hot part is n - p - 1 + m VARIABLE-base multiplications by ONE scalar (group_scale_uniform_kernel, kernels_group.hpp); everything else is
// what the library already does: the compact base arena (zkr_key_base_arena) holds the base points, the receiver path of a
// replica (arena_from_base / zkr_key_adopt_base_arena) rebuilds the window levels, the keys' MSM path multiplies their C and H
// tables by random coefficients for the check, pairing.hpp evaluates the few pairings on the host.
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "kernels_group.hpp"
#include "hostops.hpp"
#include "pairing.hpp"
#include "record_util.hpp"
#include "verify_key.hpp"
#include "zkr_internal.hpp"

namespace zkr {

// ---------------------------------------------------------------- the compare kernel
// Byte ranges of two arenas that must agree, 16 bytes per thread and step; blockIdx.y = range.  *first = smallest index of a
// range with a difference (the ranges come in the order faults are reported).
struct CmpRange {
  uint64_t off_a, off_b, units;  // units of 16 bytes (sections start 256-aligned and their slack is zeroed: arena_layout, key_build)
  uint32_t section, table;       // ZKR_KEYSEC_* and QAP side / table, for the report
};
static __global__ __launch_bounds__(256) void compare_ranges_kernel(const unsigned char *a, const unsigned char *b, const CmpRange *ranges, uint32_t *first) {
  const CmpRange r = ranges[blockIdx.y];
  const uint4 *pa = reinterpret_cast<const uint4 *>(a + r.off_a), *pb = reinterpret_cast<const uint4 *>(b + r.off_b);
  bool differ = false;
  for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < r.units; u += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 x = pa[u], y = pb[u];
    differ = differ || x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
  }
  if (differ) atomicMin(first, blockIdx.y);
}

namespace {

const char *section_name(uint32_t s) {
  static const char *const names[] = {"none", "row pointers", "columns", "wide rows", "rank map", "header", "points", "twiddles", "coefficients", "shared rank", "constants"};
  return s < sizeof(names) / sizeof(names[0]) ? names[s] : "?";
}

// *first_out = index of the first differing range, 0xffffffff when the arenas agree on all of them
int compare_ranges(int device, const unsigned char *a, const unsigned char *b, const std::vector<CmpRange> &ranges, uint32_t *first_out) {
  ZKR_HIP_CHECK(hipSetDevice(device));
  DevBuf dr, df;
  int rc;
  if ((rc = dr.alloc(ranges.size() * sizeof(CmpRange))) || (rc = df.alloc(4))) return rc;
  const uint32_t none = 0xffffffffu;
  ZKR_HIP_CHECK(hipMemcpy(dr.p, ranges.data(), ranges.size() * sizeof(CmpRange), hipMemcpyHostToDevice));
  ZKR_HIP_CHECK(hipMemcpy(df.p, &none, 4, hipMemcpyHostToDevice));
  compare_ranges_kernel<<<dim3(1024, (unsigned)ranges.size()), 256>>>(a, b, dr.as<CmpRange>(), df.as<uint32_t>());
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpy(first_out, df.p, 4, hipMemcpyDeviceToHost));
  return 0;
}
CmpRange range_of(uint64_t off_a, uint64_t off_b, uint64_t bytes, uint32_t section, uint32_t table) { return CmpRange{off_a, off_b, (bytes + 15) / 16, section, table}; }


// record layout (ZKR_CONTRIBUTION_BYTES): delta1_before | delta1_after | delta2_after | R | z
constexpr size_t REC_D1B = 0, REC_D1A = 64, REC_D2A = 128, REC_R = 256, REC_Z = 320;
// the Schnorr challenge: the library's host MiMC sponge over the ten coordinates the proof binds
int challenge(const uint8_t *d1b, const uint8_t *d1a, const uint8_t *d2a, const uint8_t *r, uint8_t c_out[32]) {
  uint8_t in[320];
  memcpy(in, d1b, 64); memcpy(in + 64, d1a, 64); memcpy(in + 128, d2a, 128); memcpy(in + 256, r, 64);
  return zkr_mimcsponge_multihash(in, 10, c_out);
}

struct Parsed {
  G1Affine d1b, d1a, r;
  G2Affine d2a;
};
// everything zkr_contribution_check states; `why` names what failed
bool record_valid(const uint8_t *rec, Parsed &p, const char **why) {
  if (!read_g1_std(rec + REC_D1B, p.d1b) || !read_g1_std(rec + REC_D1A, p.d1a) || !read_g1_std(rec + REC_R, p.r)) { *why = "a G1 member is at infinity, out of range or off the curve"; return false; }
  if (!read_g2_std(rec + REC_D2A, p.d2a)) { *why = "delta2_after is not a member of G2"; return false; }
  if (memcmp(rec + REC_D1B, rec + REC_D1A, 64) == 0) { *why = "delta did not move"; return false; }
  if (!lt_words(rec + REC_Z, FrParams::P)) { *why = "z is not below r"; return false; }
  uint8_t c[32];
  if (challenge(rec + REC_D1B, rec + REC_D1A, rec + REC_D2A, rec + REC_R, c)) { *why = "challenge hash failed"; return false; }
  if (!schnorr_verify(p.d1b, p.d1a, p.r, rec + REC_Z, c)) { *why = "the proof of knowledge of d does not verify"; return false; }
  if (!pairings_equal(p.d1a, g2_generator(), g1_generator(), p.d2a)) { *why = "delta1_after and delta2_after are not the same multiple of the generators"; return false; }
  return true;
}


// everything that reveals d: wiped however zkr_key_contribute is left
struct Secrets {
  U256 d, dinv, nonce;
  Fr dm, tmp;
  ResponseScratch resp;  // wipes itself
  uint32_t naf[16];
  DevBuf d_naf;
  ~Secrets() {
    if (d_naf.p) { (void)hipMemset(d_naf.p, 0, sizeof(naf)); (void)hipDeviceSynchronize(); }
    explicit_bzero(&d, sizeof(d)); explicit_bzero(&dinv, sizeof(dinv)); explicit_bzero(&nonce, sizeof(nonce));
    explicit_bzero(&dm, sizeof(dm)); explicit_bzero(&tmp, sizeof(tmp)); explicit_bzero(naf, sizeof(naf));
  }
};

int refuse_shard(const zkr_key *key, const char *what) {
  if (key->h.shard_parts <= 1) return 0;
  set_error("%s: this key is shard %u of %u of a proving key; it takes a whole key", what, key->h.shard_part, key->h.shard_parts);
  return ZKR_ERR_ARG;
}

int scale_table(G1Affine *pts, uint32_t n, const uint32_t *d_naf, int top, Fq *ztmp) {
  if (!n) return 0;
  int npt;
  const unsigned grid = group_scale_grid(n, &npt);
  group_scale_uniform_kernel<G1C><<<grid, GROUP_THREADS>>>(pts, n, npt, d_naf, top, ztmp);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace

// two device buffers of `bytes` (a multiple of 16) hold the same bytes: the compare kernel over one range (zkr_internal.hpp)
int device_bytes_equal(int device, const void *a, const void *b, size_t bytes, bool *same) {
  uint32_t first = 0;
  if (int rc = compare_ranges(device, (const unsigned char *)a, (const unsigned char *)b, {CmpRange{0, 0, bytes / 16, 0, 0}}, &first)) return rc;
  *same = first == 0xffffffffu;
  return 0;
}
}  // namespace zkr

using namespace zkr;

extern "C" {

int zkr_contribution_check(const uint8_t record[ZKR_CONTRIBUTION_BYTES], int *valid) {
  if (!record || !valid) { set_error("null argument"); return ZKR_ERR_ARG; }
  Parsed p;
  const char *why = "";
  *valid = record_valid(record, p, &why) ? 1 : 0;
  if (!*valid) set_error("contribution record: %s", why);
  return 0;
}

int zkr_vk_contribute(const void *vk_bin, size_t vk_len, const uint8_t record[ZKR_CONTRIBUTION_BYTES], void **vk_out, size_t *vk_out_len) {
  if (!vk_bin || !record || !vk_out || !vk_out_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  const uint8_t *vk = (const uint8_t *)vk_bin;
  const size_t fixed = VK_FIXED_BYTES;
  const uint32_t n_ic = vk_len >= fixed ? vk_ic_count(vk) : 0;
  if (vk_len < fixed || vk_len != fixed + 64ull * n_ic) { set_error("verifying key length %zu does not match its IC count", vk_len); return ZKR_ERR_ARG; }
  Parsed p;
  const char *why = "";
  if (!record_valid(record, p, &why)) { set_error("contribution record: %s", why); return ZKR_ERR_ARG; }
  G2Affine vk_delta2;
  if (!read_g2_std(vk + VK_OFF_DELTA2, vk_delta2)) { set_error("vk_delta_2 is not a member of G2"); return ZKR_ERR_ARG; }
  if (!pairings_equal(p.d1b, g2_generator(), g1_generator(), vk_delta2)) { set_error("the record does not continue this verifying key (its delta1_before is not this key's delta)"); return ZKR_ERR_ARG; }
  std::vector<uint8_t> next(vk, vk + vk_len);
  memcpy(next.data() + VK_OFF_DELTA2, record + REC_D2A, 128);
  return give_bytes(next, vk_out, vk_out_len);
}

int zkr_key_contribute(const zkr_key *key, const uint8_t *d32, zkr_key **out, uint8_t record_out[ZKR_CONTRIBUTION_BYTES]) {
  if (!key || !out || !record_out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rs = refuse_shard(key, "zkr_key_contribute")) return rs;
  Secrets s;
  int rc;
  if (d32) {
    if (!valid_secret(d32)) { set_error("zkr_key_contribute: d must satisfy 1 < d < r"); return ZKR_ERR_ARG; }
    memcpy(s.d.v, d32, 32);
  } else if ((rc = draw_secret(s.d))) return rc;
  if ((rc = draw_secret(s.nonce))) return rc;
  memcpy(s.dm.v, s.d.v, 32);
  s.dm = to_mont(s.dm);
  s.tmp = from_mont(inv(s.dm));
  memcpy(s.dinv.v, s.tmp.v, 32);
  const int top = naf_of(s.dinv, s.naf, s.naf + 8);

  // the new delta and the record (host; a few hundred group operations)
  const ArenaHeader &h = key->h;
  const G1Affine d1b = load_g1(h.delta1);
  const G2Affine d2b = load_g2(h.delta2);
  const G1XYZZ d1a_x = scalar_mul(to_xyzz(d1b), s.d);
  const G2XYZZ d2a_x = scalar_mul(to_xyzz(d2b), s.d);
  const G1XYZZ r_x = scalar_mul(to_xyzz(d1b), s.nonce);
  if (d1b.is_inf() || d1a_x.is_inf() || d2a_x.is_inf() || r_x.is_inf()) { set_error("zkr_key_contribute: the key's delta is not a point of order r"); return ZKR_ERR_BAD_KEY; }
  const G1Affine d1a = to_affine(d1a_x), r_pt = to_affine(r_x);
  const G2Affine d2a = to_affine(d2a_x);
  uint8_t rec[ZKR_CONTRIBUTION_BYTES];
  store_g1_std(rec + REC_D1B, d1b); store_g1_std(rec + REC_D1A, d1a); store_g2_std(rec + REC_D2A, d2a); store_g1_std(rec + REC_R, r_pt);
  uint8_t c[32];
  if ((rc = challenge(rec + REC_D1B, rec + REC_D1A, rec + REC_D2A, rec + REC_R, c))) return rc;
  schnorr_response(s.nonce, c, s.dm, s.resp, rec + REC_Z);

  // a device copy of the compact arena (the key's own is cached on it and stays as it is): scale C and H there, patch delta
  void *base = nullptr;
  size_t base_len = 0;
  if ((rc = zkr_key_base_arena(const_cast<zkr_key *>(key), &base, &base_len))) return rc;
  ZKR_HIP_CHECK(hipSetDevice(key->device));
  ArenaHeader b;
  base_layout(h, b);
  DevBuf copy, ztmp;
  const uint32_t n_max = h.npts[T_C] > h.npts[T_H] ? h.npts[T_C] : h.npts[T_H];
  if ((rc = copy.alloc(base_len)) || (rc = ztmp.alloc((size_t)n_max * 2 * sizeof(Fq))) || (rc = s.d_naf.alloc(sizeof(s.naf)))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(copy.p, base, base_len, hipMemcpyDeviceToDevice));
  ZKR_HIP_CHECK(hipMemcpy(s.d_naf.p, s.naf, sizeof(s.naf), hipMemcpyHostToDevice));
  unsigned char *cb = copy.as<unsigned char>();
  for (int t : {T_C, T_H})
    if ((rc = scale_table((G1Affine *)(cb + b.off_pts[t]), h.npts[t], s.d_naf.as<uint32_t>(), top, ztmp.as<Fq>()))) return rc;
  uint8_t consts[192];
  store_g1_mont(consts, d1a);
  store_g2_mont(consts + 64, d2a);
  ZKR_HIP_CHECK(hipMemcpy(cb + offsetof(ArenaHeader, delta1), consts, 64, hipMemcpyHostToDevice));
  ZKR_HIP_CHECK(hipMemcpy(cb + offsetof(ArenaHeader, delta2), consts + 64, 128, hipMemcpyHostToDevice));
  {
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("scaling the C and H points failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  }
  // the receiver path of a replica: THE layout, window levels, twiddles, level-0 check, workspaces
  if ((rc = zkr_key_adopt_base_arena(copy.p, base_len, key->device, out))) return rc;
  memcpy(record_out, rec, ZKR_CONTRIBUTION_BYTES);
  return 0;
}

int zkr_key_contribution_verify(const zkr_key *before, const zkr_key *after, const uint8_t record[ZKR_CONTRIBUTION_BYTES], int *valid, uint64_t report[2]) {
  if (!before || !after || !record || !valid) { set_error("null argument"); return ZKR_ERR_ARG; }
  *valid = 0;
  uint64_t rep_local[2];
  uint64_t *rep = report ? report : rep_local;
  rep[0] = rep[1] = 0;
  if (int rs = refuse_shard(before, "zkr_key_contribution_verify")) return rs;
  if (int rs = refuse_shard(after, "zkr_key_contribution_verify")) return rs;
  if (before->device != after->device) { set_error("zkr_key_contribution_verify: the keys live on devices %d and %d; replicate one to the other's", before->device, after->device); return ZKR_ERR_ARG; }
  const int device = before->device;
  const ArenaHeader &hb = before->h, &ha = after->h;
  auto fail = [&](uint64_t step, uint64_t section, const char *what) {
    rep[0] = step; rep[1] = section;
    set_error("contribution verify: step %llu failed: %s", (unsigned long long)step, what);
    return 0;
  };
  // 1. the record by itself
  Parsed p;
  const char *why = "";
  if (!record_valid(record, p, &why)) return fail(1, 0, why);
  // 2. the record is about THESE keys, and delta moved by the same factor in both groups
  uint8_t m1[64], m2[128];
  store_g1_mont(m1, p.d1b);
  if (memcmp(m1, hb.delta1, 64) != 0) return fail(2, 0, "the record's delta1_before is not the first key's delta1");
  store_g1_mont(m1, p.d1a);
  store_g2_mont(m2, p.d2a);
  if (memcmp(m1, ha.delta1, 64) != 0 || memcmp(m2, ha.delta2, 128) != 0) return fail(2, 0, "the record's delta1_after / delta2_after are not the second key's");
  const G2Affine d2b = load_g2(hb.delta2);
  if (d2b.is_inf() || !pairing::g2_on_curve(d2b) || !pairing::g2_in_subgroup(d2b)) return fail(2, 0, "the first key's delta2 is not a member of G2");
  if (!pairings_equal(p.d1a, d2b, p.d1b, p.d2a)) return fail(2, 0, "delta1 and delta2 moved by different factors");
  // 3. same geometry, and everything a contribution must not touch byte-identical
  {
    bool geo = ha.total_len == hb.total_len && ha.n == hb.n && ha.p == hb.p && ha.m == hb.m && ha.logm == hb.logm && ha.nnzA == hb.nnzA && ha.nnzB == hb.nnzB && ha.tlog == hb.tlog &&
               ha.share_b == hb.share_b && ha.share_ac == hb.share_ac && ha.off_tw == hb.off_tw && ha.off_twl == hb.off_twl;
    for (int s = 0; s < 2; s++)
      geo = geo && ha.n_wide[s] == hb.n_wide[s] && ha.off_rowptr[s] == hb.off_rowptr[s] && ha.off_col[s] == hb.off_col[s] && ha.off_coef[s] == hb.off_coef[s] && ha.off_wide[s] == hb.off_wide[s];
    for (int t = 0; t < N_TABLES; t++)
      geo = geo && ha.npts[t] == hb.npts[t] && ha.win_c[t] == hb.win_c[t] && ha.rank_identity[t] == hb.rank_identity[t] && ha.off_pts[t] == hb.off_pts[t] && ha.off_rank[t] == hb.off_rank[t];
    if (!geo) return fail(3, ZKR_KEYSEC_HEADER, "the keys differ in geometry (sizes, point counts, windows)");
    if (memcmp(ha.alfa1, hb.alfa1, 64) != 0 || memcmp(ha.beta1, hb.beta1, 64) != 0 || memcmp(ha.beta2, hb.beta2, 128) != 0) return fail(3, ZKR_KEYSEC_CONSTS, "alfa1, beta1 or beta2 changed");
  }
  auto levels = [&](int t) { return (uint64_t)((255 + ha.win_c[t] - 1) / ha.win_c[t]); };
  {
    std::vector<CmpRange> rg;
    for (int s = 0; s < 2; s++) {
      const uint64_t nnz = s == 0 ? ha.nnzA : ha.nnzB;
      rg.push_back(range_of(ha.off_rowptr[s], hb.off_rowptr[s], ((uint64_t)ha.m + 1) * 4, ZKR_KEYSEC_ROWPTR, (uint32_t)s));
      rg.push_back(range_of(ha.off_col[s], hb.off_col[s], nnz * 4, ZKR_KEYSEC_COL, (uint32_t)s));
      rg.push_back(range_of(ha.off_wide[s], hb.off_wide[s], (uint64_t)ha.n_wide[s] * 4, ZKR_KEYSEC_WIDE, (uint32_t)s));
    }
    for (int t = 0; t < N_TABLES; t++) rg.push_back(range_of(ha.off_rank[t], hb.off_rank[t], (uint64_t)rank_entries(ha, t) * 4, ZKR_KEYSEC_RANK, (uint32_t)t));
    for (int t : {T_A, T_B1, T_B2}) rg.push_back(range_of(ha.off_pts[t], hb.off_pts[t], (uint64_t)ha.npts[t] * levels(t) * (t == T_B2 ? 128 : 64), ZKR_KEYSEC_POINTS, (uint32_t)t));
    rg.push_back(range_of(ha.off_tw, hb.off_tw, (uint64_t)ha.m * 32, ZKR_KEYSEC_TWIDDLES, 0));
    rg.push_back(range_of(ha.off_twl, hb.off_twl, ha.off_rowptr[0] - ha.off_twl, ZKR_KEYSEC_TWIDDLES, 1));  // the local table, up to the next section
    for (int s = 0; s < 2; s++) rg.push_back(range_of(ha.off_coef[s], hb.off_coef[s], (uint64_t)(s == 0 ? ha.nnzA : ha.nnzB) * 32, ZKR_KEYSEC_COEF, (uint32_t)s));
    uint32_t first = 0;
    if (int rc = compare_ranges(device, after->arena, before->arena, rg, &first)) return rc;
    if (first != 0xffffffffu) {
      char msg[96];
      snprintf(msg, sizeof(msg), "the %s (side / table %u) differ between the keys", section_name(rg[first].section), rg[first].table);
      return fail(3, rg[first].section, msg);
    }
  }
  // 4. the window levels of `after`'s C and H tables are what its own base points give: rebuilt, compared, freed
  {
    void *base = nullptr;
    size_t base_len = 0;
    if (int rc = zkr_key_base_arena(const_cast<zkr_key *>(after), &base, &base_len)) return rc;
    Dev<unsigned char> tmp;
    ArenaHeader ht;
    if (int rc = arena_from_base(base, base_len, device, tmp, &ht)) return rc;
    std::vector<CmpRange> rg;
    for (int t : {T_C, T_H}) rg.push_back(range_of(ha.off_pts[t], ht.off_pts[t], (uint64_t)ha.npts[t] * levels(t) * 64, ZKR_KEYSEC_POINTS, (uint32_t)t));
    uint32_t first = 0;
    if (ht.total_len != ha.total_len || ht.off_pts[T_C] != ha.off_pts[T_C] || ht.off_pts[T_H] != ha.off_pts[T_H]) return fail(4, ZKR_KEYSEC_HEADER, "the rebuilt arena has another layout");
    if (int rc = compare_ranges(device, after->arena, tmp, rg, &first)) return rc;
    if (first != 0xffffffffu) return fail(4, ZKR_KEYSEC_POINTS, first == 0 ? "the window levels of the C table are not the multiples of its base points" : "the window levels of the H table are not the multiples of its base points");
  }
  // 5. every C and H point moved by the inverse factor: random 128-bit combinations of both keys' tables (2^-128 per wrong entry)
  {
    const size_t nw = rank_entries(ha, T_C), nh = rank_entries(ha, T_H);
    std::vector<uint8_t> sc;
    if (int rc = random_128(sc, nw + nh)) return rc;
    ZKR_HIP_CHECK(hipSetDevice(device));
    DevBuf dsc;
    if (int rc = dsc.alloc(sc.size())) return rc;
    ZKR_HIP_CHECK(hipMemcpy(dsc.p, sc.data(), sc.size(), hipMemcpyHostToDevice));
    G1XYZZ sum[2];  // after, before
    const zkr_key *keys[2] = {after, before};
    for (int j = 0; j < 2; j++) {
      G1XYZZ c_sum, h_sum;
      if (int rc = key_table_msm(keys[j], T_C, dsc.as<Fr>(), &c_sum)) return rc;
      if (int rc = key_table_msm(keys[j], T_H, dsc.as<Fr>() + nw, &h_sum)) return rc;
      sum[j] = add_full(c_sum, h_sum);
    }
    if (sum[0].is_inf() != sum[1].is_inf()) return fail(5, 0, "the C and H points did not move by the inverse of delta's factor");
    if (!sum[0].is_inf() && !pairings_equal(to_affine(sum[0]), p.d2a, to_affine(sum[1]), d2b)) return fail(5, 0, "the C and H points did not move by the inverse of delta's factor");
  }
  *valid = 1;
  return 0;
}

}  // extern "C"
