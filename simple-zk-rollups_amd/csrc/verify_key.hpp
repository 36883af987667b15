// verify_key.hpp -- the verifying key as the verifiers read it: THE parser of vk_bin (include/zkr.h, zkr_verify) with its bounds and
// its messages, the point readers it is built on, and the 8-bit window tables of the IC points.  Host only.  Shared by the host
// verifier (zkr_verify.hip: zkr_verify, zkr_verify_batch) and the device one (zkr_verify_gpu.hip: zkr_vk_load), so that both
// refuse the same keys in the same words.
#pragma once
#include <string.h>
#include <vector>
#include "pairing.hpp"
#include "zkr_internal.hpp"

namespace zkr {

inline bool fq_lt_q(const uint8_t *p) {
  uint32_t v[8];
  memcpy(v, p, 32);
  return words_below(v, FqParams::P);
}
inline bool fr_lt_r(const uint8_t *p) {
  uint32_t v[8];
  memcpy(v, p, 32);
  return words_below(v, FrParams::P);
}
// standard-form bytes -> Montgomery affine; false when a coordinate is >= q or the point is off the curve
inline bool read_g1(const uint8_t *p, G1Affine &out) {
  if (!fq_lt_q(p) || !fq_lt_q(p + 32)) return false;
  out = G1Affine{to_mont(load_fp<FqParams>(p)), to_mont(load_fp<FqParams>(p + 32))};
  return !out.is_inf() && pairing::g1_on_curve(out);
}
inline bool read_g2(const uint8_t *p, G2Affine &out) {
  for (int i = 0; i < 4; i++)
    if (!fq_lt_q(p + 32 * i)) return false;
  out = G2Affine{Fq2{to_mont(load_fp<FqParams>(p)), to_mont(load_fp<FqParams>(p + 32))},
                 Fq2{to_mont(load_fp<FqParams>(p + 64)), to_mont(load_fp<FqParams>(p + 96))}};
  // on the twist AND in the order-r subgroup (the twist has cofactor 2q - r): what precompile 8 accepts
  return !out.is_inf() && pairing::g2_on_curve(out) && pairing::g2_in_subgroup(out);
}

// vk_bin: alfa1 | beta2 | gamma2 | delta2 | u32 IC count | the IC points, standard form
constexpr size_t VK_OFF_BETA2 = 64, VK_OFF_GAMMA2 = VK_OFF_BETA2 + 128, VK_OFF_DELTA2 = VK_OFF_GAMMA2 + 128, VK_OFF_N_IC = VK_OFF_DELTA2 + 128;
constexpr size_t VK_FIXED_BYTES = VK_OFF_N_IC + 4;
// the IC count a buffer long enough for the fixed part claims
inline uint32_t vk_ic_count(const void *vk_bin) {
  uint32_t n_ic;
  memcpy(&n_ic, (const uint8_t *)vk_bin + VK_OFF_N_IC, 4);
  return n_ic;
}
// THE writer: alfa1, beta2, delta2 as a key header holds them (Montgomery affine), gamma2 and the n_ic IC points in standard form
inline void write_vk(std::vector<uint8_t> &vk, const uint8_t *alfa1_mont, const uint8_t *beta2_mont, const uint8_t *gamma2_std, const uint8_t *delta2_mont,
                     const uint8_t *ic_std, size_t n_ic) {
  vk.resize(VK_FIXED_BYTES + 64 * n_ic);
  store_g1_std(vk.data(), load_g1(alfa1_mont));
  store_g2_std(vk.data() + VK_OFF_BETA2, load_g2(beta2_mont));
  memcpy(vk.data() + VK_OFF_GAMMA2, gamma2_std, 128);
  store_g2_std(vk.data() + VK_OFF_DELTA2, load_g2(delta2_mont));
  const uint32_t n_ic32 = (uint32_t)n_ic;
  memcpy(vk.data() + VK_OFF_N_IC, &n_ic32, 4);
  memcpy(vk.data() + VK_FIXED_BYTES, ic_std, 64 * n_ic);
}
struct ParsedVk {
  G1Affine alfa1, ic0;
  G2Affine beta2, gamma2, delta2;
  std::vector<G1Affine> ics;  // IC_1 .. IC_nPublic
};
// the whole key is checked before any proof is looked at: a malformed key is an error, whatever the proofs
inline int parse_vk(const void *vk_bin, size_t vk_len, size_t n_public, ParsedVk &k) {
  const uint8_t *vk = (const uint8_t *)vk_bin;
  const size_t fixed = VK_FIXED_BYTES;
  if (vk_len < fixed) { set_error("verifying key shorter than its fixed part (%zu bytes)", fixed); return ZKR_ERR_BAD_KEY; }
  const uint32_t n_ic = vk_ic_count(vk);
  if (vk_len != fixed + 64ull * n_ic) { set_error("verifying key length %zu does not match %u IC points", vk_len, n_ic); return ZKR_ERR_BAD_KEY; }
  if (n_ic != n_public + 1) { set_error("%zu public signals for a key with %u IC points (needs nPublic + 1, TxVerifier.sol:261)", n_public, n_ic); return ZKR_ERR_ARG; }
  if (!read_g1(vk, k.alfa1) || !read_g2(vk + VK_OFF_BETA2, k.beta2) || !read_g2(vk + VK_OFF_GAMMA2, k.gamma2) || !read_g2(vk + VK_OFF_DELTA2, k.delta2) || !read_g1(vk + fixed, k.ic0)) {
    set_error("verifying key holds a point that is not on the curve (or a G2 point outside the order-r subgroup)");
    return ZKR_ERR_BAD_KEY;
  }
  k.ics.resize(n_public);
  for (size_t i = 0; i < n_public; i++)
    if (!read_g1(vk + fixed + 64 * (i + 1), k.ics[i])) { set_error("verifying key IC[%zu] is not on the curve", i + 1); return ZKR_ERR_BAD_KEY; }
  return 0;
}

// win8[i * 255 + d - 1] = d * ics[i], d = 1 .. 255, affine: 32 mixed additions per input instead of 64 full ones
inline void build_win8(const std::vector<G1Affine> &ics, std::vector<G1Affine> &win8) {
  const size_t n = ics.size();
  std::vector<G1XYZZ> pts(n * 255);
  for (size_t i = 0; i < n; i++) {
    G1XYZZ base = to_xyzz(ics[i]), cur = base;
    for (int d = 0; d < 255; d++) { pts[i * 255 + d] = cur; cur = add_mixed(cur, ics[i]); }
  }
  // affine with ONE inversion: x = X / ZZ, y = Y / ZZZ, and 1 / ZZ = ZZ^2 / ZZZ^2 (ZZ^3 = ZZZ^2), so only the ZZZ are inverted
  std::vector<Fq> pre(pts.size());
  Fq run = Fq::one();
  for (size_t j = 0; j < pts.size(); j++) {
    pre[j] = run;
    if (!pts[j].is_inf()) run = mul(run, pts[j].zzz);
  }
  Fq iv = inv(run);
  win8.assign(pts.size(), G1Affine{Fq::zero(), Fq::one()});
  for (size_t j = pts.size(); j-- > 0;) {
    if (pts[j].is_inf()) continue;  // d * IC = infinity cannot happen for a point of prime order r > 255; kept for safety
    Fq izzz = mul(iv, pre[j]);
    iv = mul(iv, pts[j].zzz);
    Fq izz = mul(sqr(pts[j].zz), sqr(izzz));
    win8[j] = G1Affine{mul(pts[j].x, izz), mul(pts[j].y, izzz)};
  }
}

}  // namespace zkr
