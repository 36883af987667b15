// crypto_program.hpp -- the rest of the reference's crypto.ts, written once for device and host: what one thread of the kernels
// of zkr_crypto.hip runs per key pair, per message or per message element, and what the host calls (zkr_mimc7_hash,
// zkr_babyjub_ecdh, zkr_mimc7_encrypt, ...) and csrc/crypto_selfcheck.cpp run without a GPU.
//   mimc7_hash / multihash   circomlib mimc7.js hash / multiHash, 91 rounds of x -> x^7
//   ecdh                     ecdh     (operator/src/utils/crypto.ts:86-93)    formatPrivKeyForBabyJub(priv) * pub, x coordinate
//   encrypt_element          encrypt  (crypto.ts:95-110)   msg[i] + hash(key, iv + i), the INTEGER sum   [DEP-KNOWLEDGE]
//   decrypt_element          decrypt  (crypto.ts:112-123)  (msg[i] - hash(key, iv + i)) mod r, msg[i] < 2r
// The round constants come through an accessor `c(i)` (Montgomery): a pointer on the host, __constant__ memory on the device,
// where every lane of a wavefront is in the same round and the index is wave-uniform.
// NOT constant time (wallet_program.hpp says why that is accepted here).
#pragma once
#include "wallet_program.hpp"

namespace zkr {
constexpr int MIMC7_ROUNDS = 91;
constexpr uint32_t CRYPTO_MAX_ARITY = 65536;

struct Mimc7ConstPtr {  // the host's accessor (and any caller's that holds the table in memory)
  const Fr *p;
  ZKR_HD Fr operator()(int i) const { return p[i]; }
};

ZKR_HD Fr cr_pow7(const Fr &t) {  // four products
  const Fr t2 = sqr(t), t4 = sqr(t2);
  return mul(mul(t4, t2), t);
}
// hash(x, k): t_0 = x + k, t_i = t_{i-1}^7 + k + c_i, result t_90^7 + k.  364 products.
template <class C>
ZKR_HD Fr cr_mimc7_hash(const C &c, const Fr &x, const Fr &k) {
  Fr t = add(x, k);
#pragma unroll 1
  for (int i = 1; i < MIMC7_ROUNDS; i++) t = add(add(cr_pow7(t), k), c(i));
  return add(cr_pow7(t), k);
}
// one step of multiHash(arr, key): r = r + a + hash(a, r), r starting from the key
template <class C>
ZKR_HD Fr cr_mimc7_absorb(const C &c, const Fr &r, const Fr &a) {
  return add(add(r, a), cr_mimc7_hash(c, a, r));
}
// multiHash over n standard-form elements below r (the caller has checked them); Montgomery out
template <class C>
ZKR_HD Fr cr_mimc7_multihash(const C &c, const Fr *in, uint32_t n, const Fr &key) {
  Fr r = key;
#pragma unroll 1
  for (uint32_t i = 0; i < n; i++) r = cr_mimc7_absorb(c, r, to_mont(in[i]));
  return r;
}

// ------------------------------------------------------------------------------------------------ ecdh
ZKR_HD uint32_t cr_take_high_bit(uint32_t (&w)[8]) {  // the highest bit of a 256-bit number, which then moves up by one
  const uint32_t b = w[7] >> 31;
#pragma unroll
  for (int i = 7; i > 0; i--) w[i] = (w[i] << 1) | (w[i - 1] >> 31);
  w[0] <<= 1;
  return b;
}
// e * (px, py) for e < 2^253 (e is used up), from the top bit down: a doubling and an addition of the point or of the identity
// per bit, so the lanes of a wavefront stay in step.  The law is complete: any point of the curve, the identity and the
// low-order points included, and Z never 0.
ZKR_HD PtD cr_mul_any(const TxConsts &k, uint32_t (&e)[8], const Fr &px, const Fr &py) {
  const Fr one = Fr::one(), zero = Fr::zero();
  PtD acc{zero, one, one};
#pragma unroll
  for (int i = 0; i < 3; i++) cr_take_high_bit(e);  // bits 255..253 are clear
#pragma unroll 1
  for (int i = 0; i < 253; i++) {
    const uint32_t bit = cr_take_high_bit(e);
    acc = bj_dbl(k.a, acc);
    acc = bj_add_affine(k.a, k.d, acc, wl_pick(bit, px, zero), wl_pick(bit, py, one));
  }
  return acc;
}
// ecdh(priv, pub): priv, px, py Montgomery; the shared key (Montgomery)
ZKR_HD Fr cr_ecdh(const TxConsts &k, const Fr &priv, const Fr &px, const Fr &py) {
  uint32_t f[8];
  wl_format_privkey(k, priv, f);
  const PtD a = cr_mul_any(k, f, px, py);
  return mul(a.x, inv_inline(a.z));
}

// ------------------------------------------------------------------------------------------------ the cipher
// hash(key, (iv + i) mod r): element i of the keystream; key and iv Montgomery, i < 2^32
template <class C>
ZKR_HD Fr cr_keystream(const C &c, const Fr &key, const Fr &iv, uint32_t i) {
  return cr_mimc7_hash(c, key, add(iv, wl_small(i)));
}
// m + ks as integers: both below r < 2^254, so the sum (up to 2r - 2) fits the eight words.  m standard form, ks Montgomery.
ZKR_HD Fr cr_encrypt_element(const Fr &m, const Fr &ks) {
  const Fr s = from_mont(ks);
  Fr o;
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t v = (uint64_t)m.v[i] + s.v[i] + carry;
    o.v[i] = (uint32_t)v;
    carry = v >> 32;
  }
  return o;
}
// (e - ks) mod r for e < 2r (standard form): r comes off once if it must, then the field's subtraction.  Standard form out.
ZKR_HD Fr cr_decrypt_element(const Fr &e, const Fr &ks) {
  Fr d;
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t v = (uint64_t)e.v[i] - FrParams::P[i] - br;
    d.v[i] = (uint32_t)v;
    br = (v >> 63) & 1;
  }
  const uint32_t keep = 0u - (uint32_t)br;  // e < r: keep e
#pragma unroll
  for (int i = 0; i < 8; i++) d.v[i] = (e.v[i] & keep) | (d.v[i] & ~keep);
  return from_mont(sub(to_mont(d), ks));
}
// a ciphertext element is below 2r (standard form)?
ZKR_HD bool cr_below_2r(const Fr &e) {
  uint32_t two_r[8];
#pragma unroll
  for (int i = 7; i > 0; i--) two_r[i] = (FrParams::P[i] << 1) | (FrParams::P[i - 1] >> 31);
  two_r[0] = FrParams::P[0] << 1;
  return words_below(e.v, two_r);
}
}  // namespace zkr
