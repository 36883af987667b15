// curve29_raw.hpp -- the group law of curve29.hpp on RAW limbs, for the self tests of both builds: the host shim
// (host_arith_shim.cpp zkt29_curve_raw) and the device hook (zkr_selftest.hip zkr_selftest_curve29) run the same function on the
// same records, so a test can put an accumulator's coordinates AT the bounds its type declares -- values no entry point of the
// product can inject -- and compare either build with integer arithmetic, and the two with each other limb for limb.
//
// A coordinate is 9 limbs over Fq (G1) and 18 over Fq2 (G2: re, im): the low eight below 2^29, the top limb = value >> 232; values
// x 2^261.  A record is the operation's coordinates in the order below, then two flag words; nothing is reduced on the way in or out.
//   op 0  add_mixed29(acc, q, neg_q)           X Y ZZ ZZZ | qx qy       flags: neg_q, -        out: X Y ZZ ZZZ
//   op 1  add_affine_affine29(a, na, b, nb)    ax ay | bx by            flags: neg_a, neg_b    out: X Y ZZ ZZZ
//   op 2  add_full29(a, b, again)              a: X Y ZZ ZZZ | b: ...   (device: again() reads b from the record again)
//   op 3  dbl_xyzz29(p)                        X Y ZZ ZZZ
//   op 4  dbl_affine29(x, y)                   x y
//   op 5  dbl_jac29(p)                         X Y Z                                           out: X Y Z
//   op 6  pack_xyzz(p), unpack_xyzz of that    X Y ZZ ZZZ                                      out: the packed words (8 / 16 per
//                                                                                              coordinate), then the limbs read back
// *inf = 1 when the result is the point at infinity (its limbs are then exact zeros).
#pragma once
#include "curve29.hpp"

namespace zkr {

constexpr int CURVE29_OPS = 7;
constexpr int curve29_coords_in(int op) { return op == 0 ? 6 : op == 1 ? 4 : op == 2 ? 8 : op == 3 ? 4 : op == 4 ? 2 : op == 5 ? 3 : 4; }
constexpr int curve29_limbs(bool g2) { return g2 ? 18 : 9; }
constexpr int curve29_record_words(bool g2, int op) { return curve29_coords_in(op) * curve29_limbs(g2) + 2; }
constexpr int curve29_out_words(bool g2, int op) {
  return op == 5 ? 3 * curve29_limbs(g2) : op == 6 ? 4 * (g2 ? 16 : 8) + 4 * curve29_limbs(g2) : 4 * curve29_limbs(g2);
}

template <class C> struct Raw29;
template <> struct Raw29<G1C> {
  static constexpr bool g2 = false;
  static constexpr int NL = 9, NW = 8;
  template <int H> static ZKR_HD L29<Fq29, H> load(const uint32_t *p) {
    L29<Fq29, H> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = p[i];
    return r;
  }
  template <int H> static ZKR_HD void store(uint32_t *p, const L29<Fq29, H> &x) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = x.v[i];
  }
  static ZKR_HD void store_words(uint32_t *p, const Fq &w) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = w.v[i];
  }
};
template <> struct Raw29<G2C> {
  static constexpr bool g2 = true;
  static constexpr int NL = 18, NW = 16;
  template <int H> static ZKR_HD Q29<H> load(const uint32_t *p) { return Q29<H>{Raw29<G1C>::load<H>(p), Raw29<G1C>::load<H>(p + 9)}; }
  template <int H> static ZKR_HD void store(uint32_t *p, const Q29<H> &x) { Raw29<G1C>::store(p, x.a); Raw29<G1C>::store(p + 9, x.b); }
  static ZKR_HD void store_words(uint32_t *p, const Fq2 &w) { Raw29<G1C>::store_words(p, w.a); Raw29<G1C>::store_words(p + 8, w.b); }
};

template <class C> ZKR_HD XYZZ29<C> raw_load_xyzz(const uint32_t *p) {
  using IO = Raw29<C>;
  XYZZ29<C> r;
  r.x = IO::template load<HX>(p); r.y = IO::template load<HY>(p + IO::NL);
  r.zz = IO::template load<HY>(p + 2 * IO::NL); r.zzz = IO::template load<HY>(p + 3 * IO::NL);
  return r;
}
template <class C> ZKR_HD Affine29<C> raw_load_affine(const uint32_t *p) {
  using IO = Raw29<C>;
  return Affine29<C>{IO::template load<2>(p), IO::template load<2>(p + IO::NL)};
}
template <class C> ZKR_HD void raw_store_xyzz(uint32_t *out, uint8_t *inf, const XYZZ29<C> &r) {
  using IO = Raw29<C>;
  IO::store(out, r.x); IO::store(out + IO::NL, r.y); IO::store(out + 2 * IO::NL, r.zz); IO::store(out + 3 * IO::NL, r.zzz);
  *inf = r.is_inf() ? 1 : 0;
}

// one record of operation OP: rec = curve29_record_words words, out = curve29_out_words words
template <class C, int OP>
ZKR_HD void curve29_raw_op(const uint32_t *rec, uint32_t *out, uint8_t *inf) {
  using IO = Raw29<C>;
  constexpr int NL = IO::NL;
  const uint32_t *flags = rec + curve29_coords_in(OP) * NL;
  if constexpr (OP == 0) {
    raw_store_xyzz<C>(out, inf, add_mixed29<C>(raw_load_xyzz<C>(rec), raw_load_affine<C>(rec + 4 * NL), flags[0] != 0));
  } else if constexpr (OP == 1) {
    raw_store_xyzz<C>(out, inf, add_affine_affine29<C>(raw_load_affine<C>(rec), flags[0] != 0, raw_load_affine<C>(rec + 2 * NL), flags[1] != 0));
  } else if constexpr (OP == 2) {
#if defined(__HIP_DEVICE_COMPILE__)
    raw_store_xyzz<C>(out, inf, add_full29<C>(raw_load_xyzz<C>(rec), raw_load_xyzz<C>(rec + 4 * NL), [&]() { return raw_load_xyzz<C>(rec + 4 * NL); }));
#else
    raw_store_xyzz<C>(out, inf, add_full29<C>(raw_load_xyzz<C>(rec), raw_load_xyzz<C>(rec + 4 * NL)));
#endif
  } else if constexpr (OP == 3) {
    raw_store_xyzz<C>(out, inf, dbl_xyzz29<C>(raw_load_xyzz<C>(rec)));
  } else if constexpr (OP == 4) {
    const Affine29<C> q = raw_load_affine<C>(rec);
    raw_store_xyzz<C>(out, inf, dbl_affine29<C>(q.x, q.y));
  } else if constexpr (OP == 5) {
    const Jac29<C> r = dbl_jac29<C>(Jac29<C>{IO::template load<JX>(rec), IO::template load<JY>(rec + NL), IO::template load<JZ>(rec + 2 * NL)});
    IO::store(out, r.x); IO::store(out + NL, r.y); IO::store(out + 2 * NL, r.z);
    *inf = 0;
  } else {
    const XYZZ<typename C::W> w = pack_xyzz<typename C::W>(raw_load_xyzz<C>(rec));
    IO::store_words(out, w.x); IO::store_words(out + IO::NW, w.y); IO::store_words(out + 2 * IO::NW, w.zz); IO::store_words(out + 3 * IO::NW, w.zzz);
    uint8_t again;
    raw_store_xyzz<C>(out + 4 * IO::NW, &again, unpack_xyzz(w));
    *inf = w.is_inf() ? 1 : 0;
  }
}

}  // namespace zkr
