// wprog_selfcheck.cpp -- the witness-program validator and the interpreter's host twin (wprog.hpp) in a program of their own, for
// `make wprog-asan` (AddressSanitizer + UBSan, nothing to preload).  It builds one small program that uses every opcode, runs it,
// then hands the validator every truncation of it and every single-word damage: whatever the validator ACCEPTS is run, so an
// operand it wrongly let through shows as an out-of-bounds access of the store.
#include <stdio.h>
#include <stdlib.h>
#include "wprog.hpp"

using namespace zkr;

static void put32(std::vector<uint8_t> &b, uint32_t v) { for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i))); }
static void put_const(std::vector<uint8_t> &b, uint64_t v) { for (int i = 0; i < 32; i++) b.push_back(i < 8 ? (uint8_t)(v >> (8 * i)) : 0); }

int main() {
  // inputs x, y.  wires: 0 one, 1 x, 2 y, 3 CONST 5, 4 x + y, 5 (x + y) * 5, 6 it - y, 7 INV0 of it, 8 bit 0 of x, 9 bit 253 of x,
  // 10 x - x; ASSERT_ZERO wire 10 (holds), ASSERT_ZERO wire 8 (fails for odd x)
  const uint32_t code[][4] = {{WP_CONST, 0, 0, 0}, {WP_ADD, 1, 2, 0}, {WP_MUL, 4, 3, 0}, {WP_SUB, 5, 2, 0}, {WP_INV0, 6, 0, 0}, {WP_BIT, 1, 0, 0},
                              {WP_BIT, 1, 253, 0}, {WP_SUB, 1, 1, 0}, {WP_ASSERT_ZERO, 10, 0, 0}, {WP_ASSERT_ZERO, 8, 1, 0}};
  const uint32_t n_instr = sizeof(code) / sizeof(code[0]), map[] = {0, 5, 1, 2, 7, 9};
  std::vector<uint8_t> bin;
  for (uint32_t v : {WPROG_MAGIC, WPROG_VERSION, 2u, 1u, n_instr, 6u, 1u, 2u}) put32(bin, v);
  put_const(bin, 5);
  for (const auto &in : code)
    for (uint32_t v : in) put32(bin, v);
  for (uint32_t v : map) put32(bin, v);

  WpProgram p;
  std::string err;
  if (!wprog_parse(bin.data(), bin.size(), p, err)) { fprintf(stderr, "the good program is refused: %s\n", err.c_str()); return 1; }
  if (p.n_wires != 11) { fprintf(stderr, "wire count %u, expected 11\n", p.n_wires); return 1; }
  std::vector<uint8_t> in(64, 0), wit(32 * 6), wires(32 * 11);
  uint32_t c = 9, st = 9;
  in[0] = 4; in[32] = 3;  // x = 4, y = 3: (4 + 3) * 5 = 35
  wprog_run_host(p, in.data(), wit.data(), wires.data(), &c, &st);
  if (c != WP_OK || wit[32] != 35 || wit[0] != 1 || wires[32 * 6] != 32) { fprintf(stderr, "x = 4: code %u, signal 1 = %u\n", c, wit[32]); return 1; }
  in[0] = 5;  // odd x: the second assertion fails
  wprog_run_host(p, in.data(), wit.data(), nullptr, &c, &st);
  if (c != WP_ASSERTION || st != 1 || wit[0] != 0) { fprintf(stderr, "x = 5: code %u statement %u\n", c, st); return 1; }
  memcpy(in.data(), FrParams::P, 32);  // x = r
  wprog_run_host(p, in.data(), wit.data(), wires.data(), &c, &st);
  if (c != WP_INPUT_RANGE || st != 0) { fprintf(stderr, "x = r: code %u statement %u\n", c, st); return 1; }
  in.assign(64, 0);
  in[0] = 6;

  size_t refused = 0, accepted = 0;
  auto attempt = [&](const uint8_t *b, size_t len) {
    std::vector<uint8_t> copy(b, b + len);  // exactly `len` bytes on the heap: a read past them is reported
    WpProgram q;
    std::string e;
    if (!wprog_parse(copy.data(), copy.size(), q, e)) { refused++; return; }
    accepted++;
    std::vector<uint8_t> w((size_t)32 * q.n_vars), ws((size_t)32 * q.n_wires), inputs((size_t)32 * q.n_inputs + 1, 0);
    uint32_t cc, ss;
    wprog_run_host(q, inputs.data(), w.data(), ws.data(), &cc, &ss);
  };
  for (size_t len = 0; len < bin.size(); len++) attempt(bin.data(), len);  // every truncation
  if (accepted) { fprintf(stderr, "%zu truncated programs accepted\n", accepted); return 1; }
  std::vector<uint8_t> longer(bin);
  longer.push_back(0);
  attempt(longer.data(), longer.size());
  if (accepted) { fprintf(stderr, "a program with a byte appended is accepted\n"); return 1; }
  const uint32_t values[] = {0, 1, 2, 7, 8, 10, 11, 12, 253, 254, 255, 0x0fffffffu, 0x10000000u, 0x10000001u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  for (size_t off = 0; off + 4 <= bin.size(); off += 4)  // every word of the file set to each of these
    for (uint32_t v : values) {
      std::vector<uint8_t> bad(bin);
      for (int i = 0; i < 4; i++) bad[off + i] = (uint8_t)(v >> (8 * i));
      attempt(bad.data(), bad.size());
    }
  {  // a constant equal to r
    std::vector<uint8_t> bad(bin);
    memcpy(bad.data() + WPROG_HEADER_BYTES, FrParams::P, 32);
    const size_t before = refused;
    attempt(bad.data(), bad.size());
    if (refused != before + 1) { fprintf(stderr, "a constant equal to r is accepted\n"); return 1; }
  }
  printf("wprog selfcheck ok: %zu damaged programs refused, %zu accepted and run\n", refused, accepted);
  return 0;
}
