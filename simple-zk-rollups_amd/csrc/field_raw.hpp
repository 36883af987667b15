// field_raw.hpp -- the 8 x 32-bit-limb field of field.hpp on RAW limbs, for the self tests of both builds: the host shim
// (host_arith_shim.cpp zkt_fp_raw) and the device hook (zkr_selftest.hip zkr_selftest_fp) run the same function on the same
// records.  The two builds do NOT share the code under it: the host multiplies with mul_host64 (4 x 64-bit CIOS), adds separate
// products for mul_sum2 / mul_sum4 and takes Karatsuba for the Fq2 product; the device scans product columns in a 96-bit
// accumulator (the mac96* asm statements of field.hpp and field_fused.hpp) and builds the Fq2 product and both mul_sub from the
// fused sums with negated operands.  No to_mont stands around an operation here, so an operand reaches the product with exactly
// the limbs a test chose -- the modulus itself, the quotient words all ones, the column sums at their ceiling -- and a test
// compares either build with integer arithmetic and the two with each other, bit for bit: every result is canonical.
//
// A record is 8 operands x 8 words, least significant word first (a b c d e f g h); an operation reads the first few and
// ignores the rest.  Operations, operand counts and result words: field_raw_ops.def.  The Fp operations (8 result words) run over
// Fq or Fr; the Fq2 ones (16 result words: re, im) over Fq only, their elements (re, im) pairs of operands: x = a b, y = c d,
// z = e f, w = g h.  Operand ranges are the functions' own (field.hpp): <= p for the products and the negation, < p for the rest,
// any 256-bit word for reduce_once.
#pragma once
#include <type_traits>
#include "field.hpp"

namespace zkr {

enum FieldRawOp : int {
#define ZKR_FIELD_RAW_OP(num, name, operands, out_words) FRAW_##name = num,
#include "field_raw_ops.def"
#undef ZKR_FIELD_RAW_OP
  FIELD_RAW_OPS  // one past the last
};
constexpr int FIELD_RAW_RECORD_WORDS = 64;
constexpr int field_raw_out_words(int op) {
  return 0
#define ZKR_FIELD_RAW_OP(num, name, operands, out_words) +(op == num ? out_words : 0)
#include "field_raw_ops.def"
#undef ZKR_FIELD_RAW_OP
      ;
}
constexpr bool field_raw_is_fq2(int op) { return field_raw_out_words(op) == 16; }
// what a caller may ask for: a listed op, field 0 = Fq or 1 = Fr, the Fq2 ops over Fq only
constexpr bool field_raw_valid(int field, int op) { return op >= 0 && op < FIELD_RAW_OPS && (field == 0 || (field == 1 && !field_raw_is_fq2(op))); }

template <class PM> ZKR_HD Fp<PM> raw_load_fp(const uint32_t *rec, int k) {  // operand k of a record
  Fp<PM> r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = rec[8 * k + i];
  return r;
}
template <class PM> ZKR_HD void raw_store_fp(uint32_t *p, const Fp<PM> &x) {
#pragma unroll
  for (int i = 0; i < 8; i++) p[i] = x.v[i];
}
ZKR_HD Fq2 raw_load_fq2(const uint32_t *rec, int k) { return Fq2{raw_load_fp<FqParams>(rec, 2 * k), raw_load_fp<FqParams>(rec, 2 * k + 1)}; }
ZKR_HD void raw_store_fq2(uint32_t *p, const Fq2 &x) { raw_store_fp(p, x.a); raw_store_fp(p + 8, x.b); }

// one record of operation OP: rec = FIELD_RAW_RECORD_WORDS words, out = field_raw_out_words(OP) words
template <class PM, int OP>
ZKR_HD void field_raw_op(const uint32_t *rec, uint32_t *out) {
  static_assert(OP >= 0 && OP < FIELD_RAW_OPS, "an operation of field_raw_ops.def");
  static_assert(!field_raw_is_fq2(OP) || std::is_same<PM, FqParams>::value, "Fq2 stands over Fq");
#define ZKR_RAW(k) raw_load_fp<PM>(rec, k)
  if constexpr (OP == FRAW_mul) raw_store_fp(out, mul(ZKR_RAW(0), ZKR_RAW(1)));
  else if constexpr (OP == FRAW_sqr) raw_store_fp(out, sqr(ZKR_RAW(0)));
  else if constexpr (OP == FRAW_add) raw_store_fp(out, add(ZKR_RAW(0), ZKR_RAW(1)));
  else if constexpr (OP == FRAW_sub) raw_store_fp(out, sub(ZKR_RAW(0), ZKR_RAW(1)));
  else if constexpr (OP == FRAW_neg) raw_store_fp(out, neg(ZKR_RAW(0)));
  else if constexpr (OP == FRAW_reduce_once) raw_store_fp(out, reduce_once(ZKR_RAW(0)));
  else if constexpr (OP == FRAW_mul_sum2) raw_store_fp(out, mul_sum2(ZKR_RAW(0), ZKR_RAW(1), ZKR_RAW(2), ZKR_RAW(3)));
  else if constexpr (OP == FRAW_mul_sum4) raw_store_fp(out, mul_sum4(ZKR_RAW(0), ZKR_RAW(1), ZKR_RAW(2), ZKR_RAW(3), ZKR_RAW(4), ZKR_RAW(5), ZKR_RAW(6), ZKR_RAW(7)));
  else if constexpr (OP == FRAW_mul_sub) raw_store_fp(out, mul_sub(ZKR_RAW(0), ZKR_RAW(1), ZKR_RAW(2), ZKR_RAW(3)));
  else if constexpr (OP == FRAW_to_mont) raw_store_fp(out, to_mont(ZKR_RAW(0)));
  else if constexpr (OP == FRAW_from_mont) raw_store_fp(out, from_mont(ZKR_RAW(0)));
  else if constexpr (OP == FRAW_inv) raw_store_fp(out, inv(ZKR_RAW(0)));
  else if constexpr (OP == FRAW_fq2_mul) raw_store_fq2(out, mul(raw_load_fq2(rec, 0), raw_load_fq2(rec, 1)));
  else if constexpr (OP == FRAW_fq2_sqr) raw_store_fq2(out, sqr(raw_load_fq2(rec, 0)));
  else if constexpr (OP == FRAW_fq2_mul_sub) raw_store_fq2(out, mul_sub(raw_load_fq2(rec, 0), raw_load_fq2(rec, 1), raw_load_fq2(rec, 2), raw_load_fq2(rec, 3)));
  else raw_store_fq2(out, inv(raw_load_fq2(rec, 0)));
#undef ZKR_RAW
}

// operation `op` (checked by the caller: field_raw_valid) as one call f(std::integral_constant<int, OP>) -- the switch of both
// builds; an Fq2 op over Fr is never instantiated
template <class PM, class F>
inline void field_raw_dispatch(int op, F &&f) {
  switch (op) {
#define ZKR_FIELD_RAW_OP(num, name, operands, out_words) \
  case num:                                               \
    if constexpr (out_words == 8 || std::is_same<PM, FqParams>::value) f(std::integral_constant<int, num>());  \
    break;
#include "field_raw_ops.def"
#undef ZKR_FIELD_RAW_OP
    default: break;
  }
}

}  // namespace zkr
