// hostops.hpp -- small host-side group operations shared by the proof assembly (zkr_api.hip) and the
// CPU arithmetic test shim.  Uses the same field/curve templates as the device code.
#pragma once
#include <string.h>
#include <vector>
#include "curve.hpp"

namespace zkr {

struct U256 {
  uint32_t v[8];
};
static inline U256 load_u256(const uint8_t *p) { U256 r; memcpy(r.v, p, 32); return r; }

template <class PM>
static inline Fp<PM> load_fp(const uint8_t *p) { Fp<PM> r; memcpy(r.v, p, 32); return r; }
template <class PM>
static inline void store_fp(uint8_t *p, const Fp<PM> &a) { memcpy(p, a.v, 32); }

static inline G1Affine load_g1(const uint8_t *p) { return G1Affine{load_fp<FqParams>(p), load_fp<FqParams>(p + 32)}; }
static inline G2Affine load_g2(const uint8_t *p) {
  return G2Affine{Fq2{load_fp<FqParams>(p), load_fp<FqParams>(p + 32)}, Fq2{load_fp<FqParams>(p + 64), load_fp<FqParams>(p + 96)}};
}

// the generators (Montgomery affine): G1 (1, 2), TxVerifier.sol:24-26; G2 in snarkjs order [re, im] (TxVerifier.sol:30-35 lists [im, re])
static inline G1Affine g1_generator() { return G1Affine{Fq::one(), add(Fq::one(), Fq::one())}; }
static inline G2Affine g2_generator() {
  static const uint32_t GX0[8] = {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu};
  static const uint32_t GX1[8] = {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u};
  static const uint32_t GY0[8] = {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u};
  static const uint32_t GY1[8] = {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};
  G2Affine g;
  memcpy(g.x.a.v, GX0, 32); memcpy(g.x.b.v, GX1, 32); memcpy(g.y.a.v, GY0, 32); memcpy(g.y.b.v, GY1, 32);
  g.x.a = to_mont(g.x.a); g.x.b = to_mont(g.x.b); g.y.a = to_mont(g.y.a); g.y.b = to_mont(g.y.b);
  return g;
}

// k * P, k a 256-bit standard-form integer (left-to-right double-and-add)
template <class F>
static inline XYZZ<F> scalar_mul(const XYZZ<F> &p, const U256 &k) {
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int i = 255; i >= 0; i--) {
    acc = dbl_xyzz(acc);
    if ((k.v[i >> 5] >> (i & 31)) & 1) acc = add_full(acc, p);
  }
  return acc;
}

// affine standard-form bytes (x,y[,..]) of a non-infinity point
static inline void store_g1_std(uint8_t *out, const G1Affine &a) {
  store_fp(out, from_mont(a.x));
  store_fp(out + 32, from_mont(a.y));
}
static inline void store_g2_std(uint8_t *out, const G2Affine &a) {
  store_fp(out, from_mont(a.x.a));
  store_fp(out + 32, from_mont(a.x.b));
  store_fp(out + 64, from_mont(a.y.a));
  store_fp(out + 96, from_mont(a.y.b));
}

// ---- proof assembly helpers (host): 4-bit windows over 256-bit standard-form scalars ----------------------------
static inline uint32_t nibble(const U256 &k, int i) { return (k.v[i >> 3] >> ((i & 7) * 4)) & 15; }

// Fixed base (delta_1, delta_2 of a key): tab[15 * i + d - 1] = d * 16^i * P, affine, for i < 64, d = 1..15, so
// k * P is at most 64 mixed additions.  Built once per key.
template <class F>
static inline std::vector<Affine<F>> fixed_base_table(const Affine<F> &p) {
  std::vector<XYZZ<F>> pts;
  pts.reserve(64 * 15);
  XYZZ<F> base = to_xyzz(p);
  for (int i = 0; i < 64; i++) {
    XYZZ<F> acc = base;
    for (int d = 1; d <= 15; d++) {
      pts.push_back(acc);
      acc = add_full(acc, base);
    }
    base = acc;  // 16 * base
  }
  std::vector<Affine<F>> tab(pts.size());
  for (size_t j = 0; j < pts.size(); j++) tab[j] = to_affine(pts[j]);
  return tab;
}
template <class F>
static inline XYZZ<F> fixed_base_mul(const std::vector<Affine<F>> &tab, const U256 &k) {
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int i = 0; i < 64; i++) {
    uint32_t d = nibble(k, i);
    if (d && !tab[15 * i + d - 1].is_inf()) acc = add_mixed(acc, tab[15 * i + d - 1]);
  }
  return acc;
}
// a * P + b * Q with shared doublings (two variable bases: the MSM results the blinding multiplies)
template <class F>
static inline XYZZ<F> double_scalar_mul(const XYZZ<F> &p, const U256 &a, const XYZZ<F> &q, const U256 &b) {
  XYZZ<F> tp[16], tq[16];
  tp[0] = tq[0] = XYZZ<F>::inf();
  for (int d = 1; d < 16; d++) {
    tp[d] = add_full(tp[d - 1], p);
    tq[d] = add_full(tq[d - 1], q);
  }
  XYZZ<F> acc = XYZZ<F>::inf();
  for (int i = 63; i >= 0; i--) {
    if (!acc.is_inf())
      for (int j = 0; j < 4; j++) acc = dbl_xyzz(acc);
    uint32_t da = nibble(a, i), db = nibble(b, i);
    if (da) acc = add_full(acc, tp[da]);
    if (db) acc = add_full(acc, tq[db]);
  }
  return acc;
}

}  // namespace zkr
