// wallet_selfcheck.cpp -- a stand-alone program over the host build of the wallet programs (wallet_program.hpp: format_privkey,
// pubkey, sign, the withdraw witness), meant for a sanitizer build (`make wallet-asan`: AddressSanitizer + UBSan on this file and
// rollup.cpp; no Python and no HIP in the process).  It runs the programs over the case list of tests/test_wallet_cpu.py -- keys 0,
// 1 and r - 1, the reference's two key pairs, one key for each length the text of multiHash([priv]) takes, seeded random keys --
// with messages of arity 1, 5 and 8, and compares every result with the host calls of rollup.cpp: zkr_babyjub_format_privkey,
// zkr_babyjub_pubkey, zkr_eddsa_sign and zkr_withdraw_witness.  The witness and its workspace are allocations of exactly their
// sizes, so that a signal too many or a partial sum past the workspace is an error the sanitizer sees.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/zkr.h"
#include "wallet_program.hpp"

static char last_error[512];
namespace zkr {
void set_error(const char *fmt, ...) {  // the library's lives beside its HIP code
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof last_error, fmt, ap);
  va_end(ap);
}
bool rollup_witness_fast_host(uint32_t, uint32_t, const uint8_t *, uint8_t *) { return false; }  // rollup.cpp's witness shortcut lives in rollup_gpu.hip; unused here
void rollup_device_constants(Fr *a, Fr *d, uint32_t suborder_m1[8], Fr *b8x253, Fr *b8y253);   // rollup.cpp
const Fr *mimc_round_constants();                                                                 // rollup.cpp
}  // namespace zkr
using namespace zkr;

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fails++; fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #x, last_error); } } while (0)

static uint64_t rng_state = 0x5A4B000A;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct Elem { uint8_t b[32]; };
static Elem small(uint64_t v) {
  Elem e;
  memset(e.b, 0, 32);
  memcpy(e.b, &v, 8);
  return e;
}
static Elem below_r() {  // 253 random bits: below r
  Elem e;
  for (int i = 0; i < 4; i++) {
    const uint64_t v = rnd();
    memcpy(e.b + 8 * i, &v, 8);
  }
  e.b[31] &= 0x1F;
  return e;
}
static Elem decimal(const char *s) {
  uint32_t w[8] = {0};
  for (; *s; s++) {
    uint64_t carry = (uint64_t)(*s - '0');
    for (int i = 0; i < 8; i++) {
      const uint64_t v = (uint64_t)w[i] * 10 + carry;
      w[i] = (uint32_t)v;
      carry = v >> 32;
    }
  }
  Elem e;
  memcpy(e.b, w, 32);
  return e;
}
static int text_len(const Elem &priv) {  // hexadecimal digits of multiHash([priv])
  uint8_t h[32];
  CHECK(zkr_mimcsponge_multihash(priv.b, 1, h) == ZKR_OK);
  for (int i = 63; i > 0; i--)
    if ((h[i >> 1] >> ((i & 1) * 4)) & 15) return i + 1;
  return 1;
}
static Fr as_fr(const uint8_t *p) {
  Fr a;
  memcpy(a.v, p, 32);
  return a;
}

int main() {
  std::vector<Fr> tab(2 * 253);
  TxConsts k;
  rollup_device_constants(&k.a, &k.d, k.suborder_m1, tab.data(), tab.data() + 253);
  k.b8x = tab.data(), k.b8y = tab.data() + 253, k.mimc = mimc_round_constants();

  std::vector<Elem> keys;
  keys.push_back(small(0));
  keys.push_back(small(1));
  {
    Elem rm1;
    memcpy(rm1.b, FrParams::P, 32);
    rm1.b[0] -= 1;  // r is odd
    keys.push_back(rm1);
  }
  keys.push_back(decimal("4884893312420666846728788329068334659645814268254376926932808574485660215402"));  // tests/golden/rollup_kat.json
  keys.push_back(decimal("5571822240978976287981822894726063023722101866275711251367830831352258921143"));
  {
    bool have[3] = {false, false, false};  // texts of 64, 63 and at most 62 characters
    for (uint64_t priv = 2; priv < 5000 && !(have[0] && have[1] && have[2]); priv++) {
      const int len = text_len(small(priv)), slot = len >= 64 ? 0 : len == 63 ? 1 : 2;
      if (!have[slot]) keys.push_back(small(priv));
      have[slot] = true;
    }
    CHECK(have[0] && have[1] && have[2]);
  }
  while (keys.size() < 24) keys.push_back(below_r());

  size_t signatures = 0, witnesses = 0;
  for (const Elem &key : keys) {
    uint8_t want_f[32], want_pub[64];
    CHECK(zkr_babyjub_format_privkey(key.b, want_f) == ZKR_OK && zkr_babyjub_pubkey(key.b, want_pub) == ZKR_OK);
    const Fr ks = as_fr(key.b);
    Fr p;
    CHECK(wl_read(&ks, p));
    uint32_t f[8], formatted[8];
    wl_format_privkey(k, p, f);
    memcpy(formatted, f, 32);
    CHECK(memcmp(f, want_f, 32) == 0);
    Fr ax, ay;
    wl_pubkey(k, f, ax, ay);
    ax = from_mont(ax), ay = from_mont(ay);
    CHECK(memcmp(ax.v, want_pub, 32) == 0 && memcmp(ay.v, want_pub + 32, 32) == 0);

    for (unsigned arity : {1u, 5u, 8u}) {
      std::vector<Elem> msg(arity);  // exactly `arity` elements: the program reads no further
      for (Elem &e : msg) e = below_r();
      uint8_t want_sig[96];
      CHECK(zkr_eddsa_sign(key.b, msg[0].b, arity, want_sig) == ZKR_OK);
      std::vector<Fr> m(arity);
      memcpy(m.data(), msg.data(), (size_t)arity * 32);
      Fr r8x, r8y;
      uint32_t S[8];
      wl_sign(k, p, m.data(), arity, r8x, r8y, S);
      r8x = from_mont(r8x), r8y = from_mont(r8y);
      CHECK(memcmp(r8x.v, want_sig, 32) == 0 && memcmp(r8y.v, want_sig + 32, 32) == 0 && memcmp(S, want_sig + 64, 32) == 0);
      signatures++;
    }

    for (int which = 0; which < 3; which++) {
      Elem nul = which == 0 ? below_r() : which == 1 ? small(0) : keys[2];
      void *want = nullptr;
      size_t want_len = 0;
      CHECK(zkr_withdraw_witness((const uint8_t *)formatted, nul.b, &want, &want_len) == ZKR_OK && want_len == (size_t)WD_NVARS * 32);
      std::vector<Fr> w(WD_NVARS), ws(WD_WS_ELEMS);
      const Fr fk = as_fr((const uint8_t *)formatted), fn = as_fr(nul.b);
      const uint32_t stmt = wd_witness(k, &fk, &fn, w.data() + WD_PUBLIC, ws.data(), w.data() + 1);
      CHECK(stmt == ST_OK);
      for (uint32_t s = 0; s < WD_NVARS; s++) w[s] = from_mont(w[s]);
      w[0] = Fr::zero(), w[0].v[0] = 1, w[3] = fn, w[4] = fk;
      CHECK(want && want_len == (size_t)WD_NVARS * 32 && memcmp(w.data(), want, want_len) == 0);
      free(want);
      witnesses++;
    }
  }
  {  // a key past 253 bits: the statement, and the host builder refuses the same key
    const Elem big = decimal("14474011154664524427946373126085988481658748083205070504932198000989141204992");  // 2^253
    const Elem nul = small(5);
    std::vector<Fr> w(WD_NVARS), ws(WD_WS_ELEMS);
    const Fr fk = as_fr(big.b), fn = as_fr(nul.b);
    CHECK(wd_witness(k, &fk, &fn, w.data() + WD_PUBLIC, ws.data(), w.data() + 1) == WD_KEY_BITS);
    CHECK(strcmp(wd_statement_text(WD_KEY_BITS), "private key fits 253 bits") == 0);
    void *want = nullptr;
    size_t want_len = 0;
    CHECK(zkr_withdraw_witness(big.b, nul.b, &want, &want_len) == ZKR_ERR_UNSATISFIED && strstr(last_error, wd_statement_text(WD_KEY_BITS)));
  }
  printf("wallet_selfcheck: %zu keys, %zu signatures, %zu witnesses, %d failures\n", keys.size(), signatures, witnesses, fails);
  return fails ? 1 : 0;
}
