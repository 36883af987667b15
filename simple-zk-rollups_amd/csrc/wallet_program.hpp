// wallet_program.hpp -- the user's side of the reference's crypto.ts and the value side of its second circuit, written once for
// device and host: what one thread of the kernels of zkr_wallet.hip runs per key, per signature or per withdraw witness, and what
// the CPU test hooks (zkr_wallet_*_program_host, zkr_withdraw_witness_program_host) and csrc/wallet_selfcheck.cpp run without a GPU.
//   format_privkey   formatPrivKeyForBabyJub  (operator/src/utils/crypto.ts:58-76)  as rollup.cpp's hex_text / pruned_secret / shr3
//   pubkey           genPublicKey             (crypto.ts:78-84)                     as rollup.cpp's pubkey_host
//   sign             sign                     (crypto.ts:143-168)                   as rollup.cpp's sign_host
//   withdraw witness Circuit.calculateWitness for withdraw.circom (operator/src/snarks/withdraw.ts:6-10): the value side of
//                    rollup.cpp's withdraw_gadget, every private signal in the host Builder's allocation order
// Scalars give up their bits from a register array that shifts: nothing here indexes a register array by a run-time value (DESIGN
// 9f: those arrays, and chains of selects, ended in scratch memory), and every function is inlined into its kernel.
// NOT constant time: the loops over text lengths, the zero tests and the memory the witness program touches depend on the
// secrets.  These programs are for a machine whose operator holds the keys anyway.
#pragma once
#include <vector>
#include "rollup_witness.hpp"

namespace zkr {
void rollup_device_constants(Fr *a, Fr *d, uint32_t suborder_m1[8], Fr *b8x253, Fr *b8y253);  // rollup.cpp
const Fr *mimc_round_constants();                                                                // rollup.cpp
// the programs' constants in HOST memory, for the host calls and the test hooks: `tab` owns the table k points into
static inline void wl_host_tables(std::vector<Fr> &tab, TxConsts &k) {
  tab.resize(2 * 253);
  rollup_device_constants(&k.a, &k.d, k.suborder_m1, tab.data(), tab.data() + 253);
  k.b8x = tab.data(), k.b8y = tab.data() + 253, k.mimc = mimc_round_constants();
}
// Withdraw(): signal 0 = 1, 1..2 = publicKey, 3 = nullifier, 4 = privateKey, then Num2Bits(253), 252 additions of six signals each
// (scalar_mul_base8) and the three-input sponge (three signals per round)
constexpr uint32_t WD_PUBLIC = 5;  // signals in front of the private ones
constexpr uint32_t WD_PRIVATE = 253 + 252 * 6 + 3 * 3 * MIMC_ROUNDS;
constexpr uint32_t WD_NVARS = WD_PUBLIC + WD_PRIVATE;
constexpr uint32_t WD_WS_PTS = 256;  // the workspace of one witness: the 252 partial sums of the fixed-base chain
constexpr uint32_t WD_WS_ELEMS = 4 * WD_WS_PTS;
// statement codes of the withdraw program: those of the pieces it shares with the transaction program (ST_INPUT_RANGE, ST_EDX,
// ST_EDY), and its own behind them
enum WdStmt : uint32_t { WD_KEY_BITS = ST_COUNT + 1 };
static inline const char *wd_statement_text(uint32_t code) {  // host
  return code == WD_KEY_BITS ? "private key fits 253 bits" : code < ST_COUNT ? TX_STMT_TEXT[code] : "";  // rollup.cpp's wording
}

// ------------------------------------------------------------------------------------------------ words
ZKR_HD uint32_t wl_take_low_bit(uint32_t (&w)[8]) {  // the lowest bit of a 256-bit number, which then moves down by one
  const uint32_t b = w[0] & 1u;
#pragma unroll
  for (int i = 0; i < 7; i++) w[i] = (w[i] >> 1) | (w[i + 1] << 31);
  w[7] >>= 1;
  return b;
}
ZKR_HD uint32_t wl_take_low_byte(uint32_t (&w)[8]) {
  const uint32_t b = w[0] & 255u;
#pragma unroll
  for (int i = 0; i < 7; i++) w[i] = (w[i] >> 8) | (w[i + 1] << 24);
  w[7] >>= 8;
  return b;
}
ZKR_HD void wl_shl4(uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 7; i > 0; i--) w[i] = (w[i] << 4) | (w[i - 1] >> 28);
  w[0] <<= 4;
}
ZKR_HD void wl_shr3(uint32_t (&s)[8]) {  // rollup.cpp shr3
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = (s[i] >> 3) | (s[i + 1] << 29);
  s[7] >>= 3;
}
ZKR_HD Fr wl_pick(uint32_t bit, const Fr &set, const Fr &clear) {  // by masks, as seq_pick
  const uint32_t m = 0u - bit;
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (set.v[i] & m) | (clear.v[i] & ~m);
  return r;
}
// standard form below r -> Montgomery; false when it is not a field element (tx_read_input, inlined)
ZKR_HD bool wl_read(const Fr *p, Fr &out) {
  const Fr a = *p;
  out = to_mont(a);
  return words_below(a.v, FrParams::P);
}
ZKR_HD Fr wl_small(uint32_t v) {  // a number below 2^32 as a field element
  Fr a = Fr::zero();
  a.v[0] = v;
  return to_mont(a);
}
// The hexadecimal digits of h as TEXT, leading zeros dropped (bigInt2Buffer, crypto.ts:20-22; rollup.cpp hex_text): byte j of
// lo (j < 32) and of hi (j - 32) is character j, zero behind the text.  Returns the text's length.  h is used up.
ZKR_HD uint32_t wl_hex_text(uint32_t (&h)[8], uint32_t (&lo)[8], uint32_t (&hi)[8]) {
  uint32_t len = 64;
  while (len > 1 && (h[7] >> 28) == 0) {
    wl_shl4(h);
    len--;
  }
#pragma unroll
  for (int half = 0; half < 2; half++) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      uint32_t word = 0;
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const uint32_t j = (uint32_t)(32 * half + 4 * i + c), nib = h[7] >> 28;
        wl_shl4(h);
        const uint32_t ch = nib < 10 ? '0' + nib : 'a' + (nib - 10);
        word |= (j < len ? ch : 0u) << (8 * c);
      }
      if (half) hi[i] = word;
      else lo[i] = word;
    }
  }
  return len;
}
// x (hi : lo, 512 bits, used up) mod m, bit-serial from the top (rollup.cpp mod_words); m < 2^255
ZKR_HD void wl_mod_words(uint32_t (&hi)[8], uint32_t (&lo)[8], const uint32_t (&m)[8], uint32_t (&r)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = 0;
#pragma unroll 1
  for (int bit = 0; bit < 512; bit++) {
    const uint32_t top = hi[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) hi[i] = (hi[i] << 1) | (hi[i - 1] >> 31);
    hi[0] = (hi[0] << 1) | (lo[7] >> 31);
#pragma unroll
    for (int i = 7; i > 0; i--) lo[i] = (lo[i] << 1) | (lo[i - 1] >> 31);
    lo[0] <<= 1;
#pragma unroll
    for (int i = 7; i > 0; i--) r[i] = (r[i] << 1) | (r[i - 1] >> 31);  // r < m < 2^255 before: nothing falls off
    r[0] = (r[0] << 1) | top;
    uint32_t d[8];
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint64_t v = (uint64_t)r[i] - m[i] - br;
      d[i] = (uint32_t)v;
      br = (v >> 63) & 1;
    }
    const uint32_t keep = 0u - (uint32_t)br;  // r < m: keep r
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = (r[i] & keep) | (d[i] & ~keep);
  }
}

// ------------------------------------------------------------------------------------------------ hash and curve
ZKR_HD void wl_feistel(const Fr *mimc, Fr &xl, Fr &xr) {  // key 0 (hasher.circom:21), no signals
#pragma unroll 1
  for (int i = 0; i < MIMC_ROUNDS; i++) {
    const Fr t = add(xl, mimc[i]);
    const Fr t2 = sqr(t);
    const Fr t5 = mul(sqr(t2), t);
    if (i < MIMC_ROUNDS - 1) {
      const Fr nl = add(xr, t5);
      xr = xl;
      xl = nl;
    } else {
      xr = add(xr, t5);
    }
  }
}
ZKR_HD Fr wl_hash1(const Fr *mimc, const Fr &x) {  // multiHash([x])
  Fr r = x, c = Fr::zero();
  wl_feistel(mimc, r, c);
  return r;
}
// e * BASE8 for e < 2^253 as ONE projective chain over the table 2^i BASE8 (e is used up).  A step whose bit is clear adds the
// identity: the lanes of a wavefront seldom all skip a step.
ZKR_HD PtD wl_mul_base8(const TxConsts &k, uint32_t (&e)[8]) {
  const Fr one = Fr::one(), zero = Fr::zero();
  PtD acc{zero, one, one};
#pragma unroll 1
  for (int i = 0; i < 253; i++) {
    const uint32_t bit = wl_take_low_bit(e);
    acc = bj_add_affine(k.a, k.d, acc, wl_pick(bit, k.b8x[i], zero), wl_pick(bit, k.b8y[i], one));
  }
  return acc;
}

// ------------------------------------------------------------------------------------------------ format_privkey, pubkey
// What a private key stands for: eddsa.pruneBuffer over the first 32 bytes of the text of multiHash([priv]) (rollup.cpp
// pruned_secret), and the text behind them, which `sign` hashes into its nonce
struct WlSecret {
  uint32_t s[8];     // the pruned secret (sign multiplies by it; the scalar of the public key is s >> 3)
  uint32_t tail[8];  // characters 32.. of the text, in order, zero behind them
  uint32_t tail_len;
};
ZKR_HD void wl_secret(const TxConsts &k, const Fr &priv, WlSecret &o) {
  const Fr h = from_mont(wl_hash1(k.mimc, priv));
  uint32_t hw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) hw[i] = h.v[i];
  const uint32_t len = wl_hex_text(hw, o.s, o.tail);
  o.tail_len = len > 32 ? len - 32 : 0;
  o.s[0] &= 0xFFFFFFF8u;                            // b[0] &= 0xF8
  o.s[7] = (o.s[7] & 0x7FFFFFFFu) | 0x40000000u;  // b[31] &= 0x7F, |= 0x40
}
// formatPrivKeyForBabyJub: priv Montgomery in, the scalar's words out
ZKR_HD void wl_format_privkey(const TxConsts &k, const Fr &priv, uint32_t (&out)[8]) {
  WlSecret sec;
  wl_secret(k, priv, sec);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = sec.s[i];
  wl_shr3(out);
}
// genPublicKey: formatted * BASE8, affine (Montgomery); formatted is used up
ZKR_HD void wl_pubkey(const TxConsts &k, uint32_t (&formatted)[8], Fr &ax, Fr &ay) {
  const PtD a = wl_mul_base8(k, formatted);
  const Fr zi = inv_inline(a.z);
  ax = mul(a.x, zi), ay = mul(a.y, zi);
}

// ------------------------------------------------------------------------------------------------ sign
// sign(prv, msg) as rollup.cpp's sign_host restates it.  msg: arity elements below r in standard form (the caller has checked
// them).  R8 Montgomery, S as words (standard form).
ZKR_HD void wl_sign(const TxConsts &k, const Fr &priv, const Fr *msg, uint32_t arity, Fr &r8x, Fr &r8y, uint32_t (&S)[8]) {
  Fr m = Fr::zero();
  {
    Fr c = Fr::zero();
    for (uint32_t i = 0; i < arity; i++) {
      Fr e;
      wl_read(msg + i, e);
      m = add(m, e);
      wl_feistel(k.mimc, m, c);
    }
  }
  WlSecret sec;
  wl_secret(k, priv, sec);
  uint32_t sub[8];  // the subgroup order: the constant of eddsa.circom:32 is order - 1 and even
#pragma unroll
  for (int i = 0; i < 8; i++) sub[i] = k.suborder_m1[i];
  sub[0] += 1;
  // r = H(h1[32:64] || msgHash as 32 little-endian bytes) mod order, the concatenation read as ONE big-endian integer
  uint32_t r[8];
  {
    const Fr k256 = wl_small(256);
    Fr pre = Fr::zero();
    for (uint32_t j = 0; j < sec.tail_len; j++) pre = add(mul(pre, k256), wl_small(wl_take_low_byte(sec.tail)));
    const Fr ms = from_mont(m);
    uint32_t mw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) mw[i] = ms.v[i];
#pragma unroll 1
    for (int j = 0; j < 32; j++) pre = add(mul(pre, k256), wl_small(wl_take_low_byte(mw)));
    const Fr hr = from_mont(wl_hash1(k.mimc, pre));
    uint32_t hw[8], lo[8], hi[8];
#pragma unroll
    for (int i = 0; i < 8; i++) hw[i] = hr.v[i];
    wl_hex_text(hw, lo, hi);  // leBuff2int of the text bytes: at most 64 of them
    wl_mod_words(hi, lo, sub, r);
  }
  // A = (s >> 3) * BASE8 and R8 = r * BASE8, one inversion for both
  Fr ax, ay;
  {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = sec.s[i];
    wl_shr3(e);
    const PtD A = wl_mul_base8(k, e);
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = r[i];
    const PtD R = wl_mul_base8(k, e);
    const Fr zi = inv_inline(mul(A.z, R.z));
    const Fr ai = mul(zi, R.z), ri = mul(zi, A.z);
    ax = mul(A.x, ai), ay = mul(A.y, ai);
    r8x = mul(R.x, ri), r8y = mul(R.y, ri);
  }
  // hm = multiHash([R8x, R8y, Ax, Ay, msgHash]);  S = (r + hm * s) mod order
  uint32_t hm[8];
  {
    Fr h = r8x, c = Fr::zero();
    wl_feistel(k.mimc, h, c);
    h = add(h, r8y);
    wl_feistel(k.mimc, h, c);
    h = add(h, ax);
    wl_feistel(k.mimc, h, c);
    h = add(h, ay);
    wl_feistel(k.mimc, h, c);
    h = add(h, m);
    wl_feistel(k.mimc, h, c);
    const Fr hs = from_mont(h);
#pragma unroll
    for (int i = 0; i < 8; i++) hm[i] = hs.v[i];
  }
  uint32_t lo[8], hi[8];  // hm * s + r < 2^254 * 2^255 + 2^251: sixteen words hold it
#pragma unroll
  for (int i = 0; i < 8; i++) lo[i] = r[i], hi[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      uint32_t &p = i + j < 8 ? lo[(i + j) & 7] : hi[(i + j) & 7];
      const uint64_t v = (uint64_t)hm[i] * sec.s[j] + p + c;
      p = (uint32_t)v;
      c = v >> 32;
    }
#pragma unroll
    for (int j = i; j < 8; j++) {  // the carry runs on through the words above
      const uint64_t v = (uint64_t)hi[j] + c;
      hi[j] = (uint32_t)v;
      c = v >> 32;
    }
  }
  wl_mod_words(hi, lo, sub, S);
}

// ------------------------------------------------------------------------------------------------ withdraw witness
// The value side of withdraw_gadget (rollup.cpp:925-937).  key, nul: standard form; w: the WD_PRIVATE private signals, in the
// Builder's allocation order (Montgomery, as the transaction program leaves them: a layout kernel or the host hook converts);
// ws: WD_WS_ELEMS workspace elements; pub: publicKey (Montgomery).  Returns the first violated statement (0: none).
ZKR_HD uint32_t wd_witness(const TxConsts &k, const Fr *key, const Fr *nul, Fr *w, Fr *ws, Fr *pub) {
  const Fr one = Fr::one(), zero = Fr::zero();
  uint32_t err = ST_OK, n = 0;
  Fr nulm;
  uint32_t e[8];
  {
    const Fr ks = *key;
    bool ok = words_below(ks.v, FrParams::P);
    ok = wl_read(nul, nulm) && ok;
    if (!ok) err = ST_INPUT_RANGE;
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = ks.v[i];
  }
  {  // Num2Bits(253) (publickeyderivation.circom:12-13): the closing constraint holds exactly when nothing is left above the bits
    uint32_t sh[8];
#pragma unroll
    for (int i = 0; i < 8; i++) sh[i] = e[i];
#pragma unroll 1
    for (int i = 0; i < 253; i++) w[n++] = wl_pick(wl_take_low_bit(sh), one, zero);
    uint32_t rest = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) rest |= sh[i];
    if (rest && !err) err = WD_KEY_BITS;
    e[7] &= (1u << (253 - 224)) - 1u;  // the bit signals are the low 253 bits
  }
  // scalar_mul_base8: the chain in projective coordinates first, one inversion, then the six signals of every addition
  Fr *wx = ws, *wy = ws + WD_WS_PTS, *wz = ws + 2 * WD_WS_PTS, *wp = ws + 3 * WD_WS_PTS;
  {
    uint32_t sh[8];
#pragma unroll
    for (int i = 0; i < 8; i++) sh[i] = e[i];
    const uint32_t b0 = wl_take_low_bit(sh);
    PtD acc{wl_pick(b0, k.b8x[0], zero), wl_pick(b0, k.b8y[0], one), one};
#pragma unroll 1
    for (int i = 1; i < 253; i++) {
      const uint32_t bit = wl_take_low_bit(sh);
      acc = bj_add_affine(k.a, k.d, acc, wl_pick(bit, k.b8x[i], zero), wl_pick(bit, k.b8y[i], one));
      wx[i - 1] = acc.x, wy[i - 1] = acc.y, wz[i - 1] = acc.z;
    }
    Fr run = one;  // rollup.cpp affine_all / batch_inverse; a complete addition never gives Z = 0
#pragma unroll 1
    for (int i = 0; i < 252; i++) {
      wp[i] = run;
      run = mul(run, wz[i]);
    }
    Fr ia = inv_inline(run);
#pragma unroll 1
    for (int i = 252; i-- > 0;) {
      const Fr zi = mul(ia, wp[i]);
      ia = mul(ia, wz[i]);
      wx[i] = mul(wx[i], zi), wy[i] = mul(wy[i], zi);
    }
  }
  PtA acc;
  {
    uint32_t sh[8];
#pragma unroll
    for (int i = 0; i < 8; i++) sh[i] = e[i];
    const uint32_t b0 = wl_take_low_bit(sh);
    acc = PtA{wl_pick(b0, k.b8x[0], zero), wl_pick(b0, k.b8y[0], one)};
#pragma unroll 1
    for (int i = 1; i < 253; i++) {  // edwards_add: beta, gamma, delta, tau, x, y
      const uint32_t bit = wl_take_low_bit(sh);
      const Fr qx = wl_pick(bit, k.b8x[i], zero), qy = wl_pick(bit, k.b8y[i], one);
      const Fr beta = mul(acc.x, qy), gamma = mul(acc.y, qx);
      const Fr delta = mul(sub(acc.y, mul(acc.x, k.a)), add(qx, qy)), tau = mul(beta, gamma);
      const Fr xv = wx[i - 1], yv = wy[i - 1];
      w[n] = beta, w[n + 1] = gamma, w[n + 2] = delta, w[n + 3] = tau, w[n + 4] = xv, w[n + 5] = yv;
      n += 6;
      const Fr dt = mul(tau, k.d);
      const bool okx = mul(add(one, dt), xv) == add(beta, gamma);
      const bool oky = mul(sub(one, dt), yv) == sub(add(delta, mul(beta, k.a)), gamma);
      if (!okx && !err) err = ST_EDX;
      if (!oky && !err) err = ST_EDY;
      acc = PtA{xv, yv};
    }
  }
  pub[0] = acc.x, pub[1] = acc.y;
  {  // multiHash([pk.x, pk.y, nullifier]) (withdraw.circom:15-19): t2, t4, x' per round
    Fr xl = zero, xr = zero;
#pragma unroll 1
    for (int part = 0; part < 3; part++) {
      xl = add(xl, part == 0 ? acc.x : part == 1 ? acc.y : nulm);
#pragma unroll 1
      for (int i = 0; i < MIMC_ROUNDS; i++) {
        const Fr t = add(xl, k.mimc[i]);
        const Fr t2 = sqr(t), t4 = sqr(t2);
        const Fr nx = add(xr, mul(t4, t));
        w[n] = t2, w[n + 1] = t4, w[n + 2] = nx;
        n += 3;
        if (i < MIMC_ROUNDS - 1) {
          xr = xl;
          xl = nx;
        } else {
          xr = nx;
        }
      }
    }
  }
  if (n != WD_PRIVATE && !err) err = ST_COUNT;
  return err;
}
}  // namespace zkr
