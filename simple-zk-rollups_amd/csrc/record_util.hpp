// record_util.hpp -- host-side reading and writing of the members of a ceremony record (zkr_contribute.hip: the delta contribution;
// zkr_ptau.hip: the powers-of-tau transcript), the Schnorr proof both records carry, and the draws from the OS CSPRNG.
#pragma once
#include <string.h>
#include <vector>
#include "hostops.hpp"
#include "pairing.hpp"
#include "zkr_internal.hpp"

namespace zkr {

// ---- host arithmetic on the record's members
static inline bool lt_words(const uint8_t *p, const uint32_t (&m)[8]) {
  uint32_t v[8];
  memcpy(v, p, 32);
  return words_below(v, m);
}
// standard-form bytes -> Montgomery affine; false for a coordinate >= q, the point at infinity or a point off its curve (G2: or
// outside the order-r subgroup, as the verifier reads G2 members)
static inline bool read_g1_std(const uint8_t *p, G1Affine &out) {
  if (!lt_words(p, FqParams::P) || !lt_words(p + 32, FqParams::P)) return false;
  out = G1Affine{to_mont(load_fp<FqParams>(p)), to_mont(load_fp<FqParams>(p + 32))};
  return !out.is_inf() && pairing::g1_on_curve(out);
}
static inline bool read_g2_std(const uint8_t *p, G2Affine &out) {
  for (int i = 0; i < 4; i++)
    if (!lt_words(p + 32 * i, FqParams::P)) return false;
  out = G2Affine{Fq2{to_mont(load_fp<FqParams>(p)), to_mont(load_fp<FqParams>(p + 32))}, Fq2{to_mont(load_fp<FqParams>(p + 64)), to_mont(load_fp<FqParams>(p + 96))}};
  return !out.is_inf() && pairing::g2_on_curve(out) && pairing::g2_in_subgroup(out);
}
static inline bool same_point(const G1XYZZ &a, const G1XYZZ &b) {
  if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
  const G1Affine x = to_affine(a), y = to_affine(b);
  return x.x == y.x && x.y == y.y;
}
// e(a, b) == e(c, d)
static inline bool pairings_equal(const G1Affine &a, const G2Affine &b, const G1Affine &c, const G2Affine &d) {
  const G1Affine ps[2] = {a, G1Affine{c.x, neg(c.y)}};
  const G2Affine qs[2] = {b, d};
  return pairing::pairing_product_is_one(ps, qs, 2);
}

static inline void store_g1_mont(uint8_t *out, const G1Affine &a) { store_fp(out, a.x); store_fp(out + 32, a.y); }
static inline void store_g2_mont(uint8_t *out, const G2Affine &a) { store_fp(out, a.x.a); store_fp(out + 32, a.x.b); store_fp(out + 64, a.y.a); store_fp(out + 96, a.y.b); }

// ---- the proof of knowledge of s with after = s before: R = k before, c = the record's challenge hash, z = k + c s mod r
// z before == R + c after (z, c: 32 bytes, standard form)
static inline bool schnorr_verify(const G1Affine &before, const G1Affine &after, const G1Affine &r, const uint8_t *z, const uint8_t *c) {
  const G1XYZZ lhs = scalar_mul(to_xyzz(before), load_u256(z));
  const G1XYZZ rhs = add_full(to_xyzz(r), scalar_mul(to_xyzz(after), load_u256(c)));
  return same_point(lhs, rhs);
}
// what a response passes through on its way to z: lives in the caller's secrets and goes with them
struct ResponseScratch {
  Fr km, prod, z;  // the nonce in Montgomery form, c s, and their sum
  ~ResponseScratch() { explicit_bzero(this, sizeof(*this)); }
};
// z_out = k + c s mod r (z itself is public); sm = s in Montgomery form
static inline void schnorr_response(const U256 &k, const uint8_t c[32], const Fr &sm, ResponseScratch &w, uint8_t z_out[32]) {
  const Fr cm = to_mont(load_fp<FrParams>(c));  // public
  memcpy(w.km.v, k.v, 32);
  w.km = to_mont(w.km);
  w.prod = mul(cm, sm);
  w.z = from_mont(add(w.km, w.prod));
  memcpy(z_out, w.z.v, 32);
}

// ---- secrets and random coefficients
static inline bool valid_secret(const uint8_t *s) {  // 1 < s < r
  bool small = s[0] <= 1;
  for (int i = 1; i < 32 && small; i++) small = s[i] == 0;
  return !small && lt_words(s, FrParams::P);
}
// draws 1 < v < r from the OS CSPRNG (rejection sampling over 254 bits)
static inline int draw_secret(U256 &v) {
  uint8_t b[32];
  int rc;
  do {
    rc = os_random(b, 32);
    b[31] &= 0x3f;
  } while (!rc && !valid_secret(b));
  if (!rc) memcpy(v.v, b, 32);
  explicit_bzero(b, sizeof(b));
  return rc;
}
// n scalars of 32 bytes, 128 random bits each: the coefficients of a random combination (2^-128 per wrong entry)
static inline int random_128(std::vector<uint8_t> &sc, size_t n) {
  sc.assign(n * 32, 0);
  std::vector<uint8_t> rnd(n * 16);
  if (int rc = os_random(rnd.data(), rnd.size())) return rc;
  for (size_t i = 0; i < n; i++) memcpy(&sc[32 * i], &rnd[16 * i], 16);
  return 0;
}

// signed binary (non-adjacent) form of e: nz bit b = digit b non-zero, sg bit b = digit b is -1; returns the leading digit's index
static inline int naf_of(const U256 &e, uint32_t nz[8], uint32_t sg[8]) {
  uint32_t k[9];
  memcpy(k, e.v, 32);
  k[8] = 0;
  memset(nz, 0, 32); memset(sg, 0, 32);
  int top = 0;
  for (int b = 0; b < 256; b++) {
    if (k[0] & 1u) {
      nz[b >> 5] |= 1u << (b & 31);
      top = b;
      if ((k[0] & 3u) == 3u) {  // digit -1: k += 1
        sg[b >> 5] |= 1u << (b & 31);
        for (int i = 0; i < 9 && ++k[i] == 0; i++) {}
      } else k[0] -= 1u;
    }
    for (int i = 0; i < 8; i++) k[i] = (k[i] >> 1) | (k[i + 1] << 31);
    k[8] >>= 1;
  }
  explicit_bzero(k, sizeof(k));
  return top;
}

}  // namespace zkr
