// crypto_selfcheck.cpp -- a stand-alone program over the host build of crypto_program.hpp (MiMC7, ecdh, the cipher's two element
// forms), meant for a sanitizer build (`make crypto-asan`: AddressSanitizer + UBSan on this file and rollup.cpp; no Python and no
// HIP in the process).  It is the known-answer table of tests/golden/mimc7_kat.json -- circomlib's constants 1 and 2 and the chain's
// 90th, go-iden3-crypto's hash(1, 2) and its three multiHash vectors, and the shared key of the reference's two key pairs
// (operator/__tests__/crypto.test.ts:22-27) -- followed by round trips of the cipher over edge and random elements, a wrapped
// counter included, in allocations of exactly their sizes.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/zkr.h"
#include "crypto_program.hpp"

static char last_error[512];
namespace zkr {
void set_error(const char *fmt, ...) {  // the library's lives beside its HIP code
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof last_error, fmt, ap);
  va_end(ap);
}
bool rollup_witness_fast_host(uint32_t, uint32_t, const uint8_t *, uint8_t *) { return false; }  // rollup.cpp's witness shortcut lives in rollup_gpu.hip; unused here
const Fr *mimc7_round_constants();  // rollup.cpp
}  // namespace zkr
using namespace zkr;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fails++; fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #x, last_error); } } while (0)

static uint64_t rng_state = 0x5A4B000C;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static Fr small(uint64_t v) {  // standard form
  Fr a = Fr::zero();
  a.v[0] = (uint32_t)v, a.v[1] = (uint32_t)(v >> 32);
  return a;
}
static Fr below_r() {  // 253 random bits, standard form
  Fr a;
  for (int i = 0; i < 8; i++) a.v[i] = (uint32_t)rnd();
  a.v[7] &= 0x1FFFFFFFu;
  return a;
}
static Fr r_minus(uint32_t k) {  // r - k, standard form
  Fr a;
  uint64_t br = k;
  for (int i = 0; i < 8; i++) {
    const uint64_t v = (uint64_t)FrParams::P[i] - br;
    a.v[i] = (uint32_t)v;
    br = (v >> 63) & 1;
  }
  return a;
}
static Fr decimal(const char *s) {
  Fr a = Fr::zero();
  for (; *s; s++) {
    uint64_t carry = (uint64_t)(*s - '0');
    for (int i = 0; i < 8; i++) {
      const uint64_t v = (uint64_t)a.v[i] * 10 + carry;
      a.v[i] = (uint32_t)v;
      carry = v >> 32;
    }
  }
  return a;
}
static Fr hex(const char *s) {
  Fr a = Fr::zero();
  for (; *s; s++) {
    const uint32_t nib = *s <= '9' ? *s - '0' : *s - 'a' + 10;
    for (int i = 7; i > 0; i--) a.v[i] = (a.v[i] << 4) | (a.v[i - 1] >> 28);
    a.v[0] = (a.v[0] << 4) | nib;
  }
  return a;
}
static bool same(const Fr &a, const Fr &b) { return memcmp(a.v, b.v, 32) == 0; }

int main() {
  const Mimc7ConstPtr c{mimc7_round_constants()};
  // the constants
  CHECK(same(from_mont(c(0)), small(0)));
  CHECK(same(from_mont(c(1)), decimal("20888961410941983456478427210666206549300505294776164667214940546594746570981")));
  CHECK(same(from_mont(c(2)), decimal("15265126113435022738560151911929040668591755459209400716467504685752745317193")));
  CHECK(same(from_mont(c(90)), decimal("13602139229813231349386885113156901793661719180900395818909719758150455500533")));
  // hash and multiHash
  CHECK(same(from_mont(cr_mimc7_hash(c, to_mont(small(1)), to_mont(small(2)))),
             decimal("10594780656576967754230020536574539122676596303354946869887184401991294982664")));
  {
    const Fr a[1] = {small(12)}, b[2] = {small(78), small(41)}, d[4] = {small(12), small(45), small(78), small(41)};
    CHECK(same(from_mont(cr_mimc7_multihash(c, a, 1, Fr::zero())), hex("237c92644dbddb86d8a259e0e923aaab65a93f1ec5758b8799988894ac0958fd")));
    CHECK(same(from_mont(cr_mimc7_multihash(c, b, 2, Fr::zero())), hex("067f3202335ea256ae6e6aadcd2d5f7f4b06a00b2d1e0de903980d5ab552dc70")));
    CHECK(same(from_mont(cr_mimc7_multihash(c, d, 4, Fr::zero())), hex("284bc1f34f335933a23a433b6ff3ee179d682cd5e5e2fcdd2d964afa85104beb")));
  }
  // ecdh: symmetric on random key pairs, whatever the keys; the public keys come from the host call
  std::vector<Fr> tab;
  TxConsts k;
  wl_host_tables(tab, k);
  {  // the reference's two key pairs (tests/golden/rollup_kat.json), each private key with the other's public key
    const Fr pa = decimal("4884893312420666846728788329068334659645814268254376926932808574485660215402");
    const Fr pb = decimal("5571822240978976287981822894726063023722101866275711251367830831352258921143");
    const Fr ax = decimal("1503249839729450699258568253188655641897688629727284476088280559686550009373");
    const Fr ay = decimal("5002035132060692260001110027450125171390191669020671174899856008595079807949");
    const Fr bx = decimal("4025550775190773106752472098712957308229408014044167272309204873490588345430");
    const Fr by = decimal("5371429479583552729106435801902737969088445564732204620785902601809639523307");
    const Fr want = decimal("6703500932075497392616036658058478666510827071759096397338988169540224393770");
    CHECK(same(from_mont(cr_ecdh(k, to_mont(pa), to_mont(bx), to_mont(by))), want));
    CHECK(same(from_mont(cr_ecdh(k, to_mont(pb), to_mont(ax), to_mont(ay))), want));
  }
  for (int round = 0; round < 6; round++) {
    const Fr pa = round == 0 ? small(0) : round == 1 ? r_minus(1) : below_r(), pb = round == 2 ? small(1) : below_r();
    uint8_t puba[64], pubb[64];
    CHECK(zkr_babyjub_pubkey((const uint8_t *)pa.v, puba) == ZKR_OK && zkr_babyjub_pubkey((const uint8_t *)pb.v, pubb) == ZKR_OK);
    Fr ax, ay, bx, by;
    memcpy(ax.v, puba, 32), memcpy(ay.v, puba + 32, 32), memcpy(bx.v, pubb, 32), memcpy(by.v, pubb + 32, 32);
    CHECK(bj_on_curve(k.a, k.d, to_mont(ax), to_mont(ay)));
    const Fr ab = cr_ecdh(k, to_mont(pa), to_mont(bx), to_mont(by)), ba = cr_ecdh(k, to_mont(pb), to_mont(ax), to_mont(ay));
    CHECK(ab == ba);
    CHECK(cr_ecdh(k, to_mont(pa), Fr::zero(), Fr::one()).is_zero());  // the identity stays the identity
  }
  // the cipher, element by element: arities 1, 5, 64 in allocations of exactly their sizes; an iv of r - 1 wraps the counter
  for (uint32_t arity : {1u, 5u, 64u}) {
    std::vector<Fr> msg(arity), enc(arity);
    for (uint32_t i = 0; i < arity; i++) msg[i] = i % 4 == 0 ? r_minus(1) : i % 4 == 1 ? small(i / 4) : below_r();
    const Fr key = to_mont(below_r());
    for (int wrap = 0; wrap < 2; wrap++) {
      const Fr iv = wrap ? to_mont(r_minus(1)) : cr_mimc7_multihash(c, msg.data(), arity, Fr::zero());
      bool past_r = false;
      for (uint32_t i = 0; i < arity; i++) {
        enc[i] = cr_encrypt_element(msg[i], cr_keystream(c, key, iv, i));
        CHECK(cr_below_2r(enc[i]));
        past_r = past_r || !words_below(enc[i].v, FrParams::P);
        CHECK(same(cr_decrypt_element(enc[i], cr_keystream(c, key, iv, i)), msg[i]));
        const Fr reduced = cr_decrypt_element(enc[i], Fr::zero());  // the same element mod r opens to the same message
        CHECK(words_below(reduced.v, FrParams::P));
        CHECK(same(cr_decrypt_element(reduced, cr_keystream(c, key, iv, i)), msg[i]));
      }
      if (arity > 1) CHECK(past_r);  // r - 1 plus a keystream element passes r
      if (wrap && arity > 1) CHECK(cr_keystream(c, key, iv, 1) == cr_mimc7_hash(c, key, Fr::zero()));  // (r - 1) + 1 = 0
    }
  }
  CHECK(cr_below_2r(r_minus(1)) && !cr_below_2r(hex("60c89ce5c263405370a08b6d0302b0ba5067d090f372e12287c3eb27e0000002")));  // 2r
  if (fails) {
    fprintf(stderr, "crypto_selfcheck: %d checks failed\n", fails);
    return 1;
  }
  printf("crypto_selfcheck: ok (constants, hash, multiHash, ecdh, cipher round trips)\n");
  return 0;
}
