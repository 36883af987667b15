// wprog.hpp -- witness programs (wprog_bin, include/zkr.h): the format's parser and validator, and THE interpreter -- one function
// that executes one instruction for one instance, written once for device and host in the way of rollup_witness.hpp.  The kernel of
// zkr_wprog.hip calls it with one lane per instance over a store laid out [wire][instance]; wprog_run_host calls it over a store
// of one instance (zkr_wprog_run_host, the CPU suite's hook).  No HIP in this file beyond the ZKR_HD qualifiers of field.hpp: the
// sanitizer program wprog_selfcheck.cpp builds it with the host compiler alone.
//
// The interpreter indexes memory with numbers taken from the program and checks none of them: wprog_parse is what makes that safe
// (every operand below the wire being defined, every constant index below the pool, every map entry below the wire count), so a
// WpProgram exists only as the output of a successful wprog_parse.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "field.hpp"

namespace zkr {

constexpr uint32_t WPROG_MAGIC = 0x50574b5au;  // "ZKWP"
constexpr uint32_t WPROG_VERSION = 1;
constexpr size_t WPROG_HEADER_BYTES = 32;
constexpr uint32_t WPROG_MAX_WIRES = 1u << 28;  // wires, constants, signals, statements: each count at most this ("fits the format")
constexpr uint32_t WPROG_BITS = 254;            // BIT takes an index below this: r < 2^254
enum WpOp : uint32_t { WP_CONST = 1, WP_ADD = 2, WP_SUB = 3, WP_MUL = 4, WP_INV0 = 5, WP_BIT = 6, WP_ASSERT_ZERO = 7 };
enum WpCode : uint32_t { WP_OK = 0, WP_INPUT_RANGE = 1, WP_ASSERTION = 2 };
constexpr uint32_t WP_NO_WIRE = 0xffffffffu;  // no wire has this number (WPROG_MAX_WIRES)

struct WpInstr { uint32_t op, a, b, c; };
static_assert(sizeof(WpInstr) == 16, "an instruction is four words");

// ---------------------------------------------------------------------------------------------------- the interpreter
// One instance.  Wire w lives at store[w * stride], Montgomery form; on the device `store` already points at the lane's column.
struct WpLane {
  Fr *store;
  size_t stride;
  const Fr *consts;   // the constant pool, Montgomery
  uint32_t next;      // the wire the next value-producing instruction defines
  uint32_t code, stmt;
  uint32_t bit_wire;  // BIT needs the standard form: the last wire it converted, and that form (num2bits asks for every bit of
  Fr bit_std;         // one wire in a row: one conversion for the run instead of one per bit)
};

ZKR_HD Fr wp_load(const Fr *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 *q = reinterpret_cast<const uint4 *>(p);  // device buffers of this unit are 16-byte aligned (checked at the entry points)
  const uint4 a = q[0], b = q[1];
  Fr r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
#else
  return *p;
#endif
}
ZKR_HD void wp_store(Fr *p, const Fr &r) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4 *q = reinterpret_cast<uint4 *>(p);
  q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
#else
  *p = r;
#endif
}
ZKR_HD Fr wp_wire(const WpLane &L, uint32_t w) { return wp_load(L.store + (size_t)w * L.stride); }

// Wire 0 and the input wires.  False with code 1 and stmt = the first input that is not below r; nothing else is written then.
ZKR_HD bool wp_begin(WpLane &L, const Fr *inputs_std, uint32_t n_inputs) {
  L.code = WP_OK;
  L.stmt = 0;
  L.bit_wire = WP_NO_WIRE;
  L.bit_std = Fr::zero();
  for (uint32_t i = 0; i < n_inputs; i++) {
    const Fr x = wp_load(inputs_std + i);
    if (!words_below(x.v, FrParams::P)) {
      L.code = WP_INPUT_RANGE;
      L.stmt = i;
      return false;
    }
  }
  wp_store(L.store, Fr::one());
  for (uint32_t i = 0; i < n_inputs; i++) wp_store(L.store + (size_t)(i + 1) * L.stride, to_mont(wp_load(inputs_std + i)));
  L.next = n_inputs + 1;
  return true;
}

// One instruction.  `in` is the same for every instance of a batch: on the device the switch is uniform over the wavefront.
ZKR_HD void wp_exec(WpLane &L, const WpInstr &in) {
  Fr v;
  switch (in.op) {
    case WP_CONST: v = wp_load(L.consts + in.a); break;
    case WP_ADD: v = add(wp_wire(L, in.a), wp_wire(L, in.b)); break;
    case WP_SUB: v = sub(wp_wire(L, in.a), wp_wire(L, in.b)); break;
    case WP_MUL: v = mul(wp_wire(L, in.a), wp_wire(L, in.b)); break;
    case WP_INV0: v = inv_inline(wp_wire(L, in.a)); break;  // a^(r-2): 0 for 0 without a branch; inline: the out-of-line inv keeps a stack frame on the device
    case WP_BIT: {
      if (L.bit_wire != in.a) {
        L.bit_std = from_mont(wp_wire(L, in.a));
        L.bit_wire = in.a;
      }
      uint32_t word = 0;  // a chain of selects: a limb indexed at run time would send the element to private memory on the device
#pragma unroll
      for (uint32_t k = 0; k < 8; k++) word = (in.b >> 5) == k ? L.bit_std.v[k] : word;
      v = (word >> (in.b & 31)) & 1 ? Fr::one() : Fr::zero();
      break;
    }
    default: {  // WP_ASSERT_ZERO: the validator lets no other opcode through
      if (L.code == WP_OK && !wp_wire(L, in.a).is_zero()) {
        L.code = WP_ASSERTION;
        L.stmt = in.b;
      }
      return;
    }
  }
  wp_store(L.store + (size_t)L.next * L.stride, v);
  L.next++;
}

// ---------------------------------------------------------------------------------------------------- parser and validator (host)
struct WpProgram {
  uint32_t n_inputs = 0, n_consts = 0, n_instr = 0, n_vars = 0, n_public = 0, n_statements = 0;
  uint32_t n_wires = 0;       // 1 + n_inputs + the value-producing instructions
  std::vector<Fr> consts;     // Montgomery
  std::vector<WpInstr> ins;
  std::vector<uint32_t> map;  // signal -> wire
};

inline uint32_t wp_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline bool wp_fail(std::string &err, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
inline bool wp_fail(std::string &err, const char *fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err = std::string("wprog_bin: ") + buf;
  return false;
}

// wprog_bin -> the program, or false and one line naming the field that is wrong.  Host only, no device call.
inline bool wprog_parse(const void *bin, size_t len, WpProgram &p, std::string &err) {
  const uint8_t *b = static_cast<const uint8_t *>(bin);
  if (len < WPROG_HEADER_BYTES) return wp_fail(err, "length is %zu bytes, shorter than the %zu-byte header", len, WPROG_HEADER_BYTES);
  const uint32_t magic = wp_le32(b), version = wp_le32(b + 4);
  if (magic != WPROG_MAGIC) return wp_fail(err, "magic is 0x%08x, not 0x%08x", magic, WPROG_MAGIC);
  if (version != WPROG_VERSION) return wp_fail(err, "version is %u, this build reads version %u", version, WPROG_VERSION);
  p.n_inputs = wp_le32(b + 8); p.n_consts = wp_le32(b + 12); p.n_instr = wp_le32(b + 16);
  p.n_vars = wp_le32(b + 20); p.n_public = wp_le32(b + 24); p.n_statements = wp_le32(b + 28);
  const struct { const char *name; uint32_t v; } counts[] = {{"n_inputs", p.n_inputs}, {"n_consts", p.n_consts}, {"n_instr", p.n_instr},
                                                             {"n_vars", p.n_vars}, {"n_statements", p.n_statements}};
  for (const auto &c : counts)
    if (c.v > WPROG_MAX_WIRES) return wp_fail(err, "%s = %u is above the format's limit %u", c.name, c.v, WPROG_MAX_WIRES);
  if ((uint64_t)1 + p.n_inputs + p.n_instr > WPROG_MAX_WIRES)
    return wp_fail(err, "n_inputs = %u and n_instr = %u give more wires than the format's limit %u", p.n_inputs, p.n_instr, WPROG_MAX_WIRES);
  const uint64_t need = WPROG_HEADER_BYTES + (uint64_t)32 * p.n_consts + (uint64_t)16 * p.n_instr + (uint64_t)4 * p.n_vars;
  if ((uint64_t)len != need) return wp_fail(err, "length is %zu bytes, the header's counts need %llu", len, (unsigned long long)need);
  if (p.n_vars == 0) return wp_fail(err, "n_vars is 0: signal 0, the constant 1, is missing");
  if (p.n_public >= p.n_vars) return wp_fail(err, "n_public = %u is not below n_vars = %u", p.n_public, p.n_vars);
  const uint8_t *q = b + WPROG_HEADER_BYTES;
  p.consts.resize(p.n_consts);
  for (uint32_t k = 0; k < p.n_consts; k++, q += 32) {
    Fr c;
    for (int i = 0; i < 8; i++) c.v[i] = wp_le32(q + 4 * i);
    if (!words_below(c.v, FrParams::P)) return wp_fail(err, "constant %u is not below r", k);
    p.consts[k] = to_mont(c);
  }
  p.ins.resize(p.n_instr);
  uint32_t wire = p.n_inputs + 1;  // the wire the instruction at hand would define
  for (uint32_t i = 0; i < p.n_instr; i++, q += 16) {
    const WpInstr in = {wp_le32(q), wp_le32(q + 4), wp_le32(q + 8), wp_le32(q + 12)};
    bool use_a = false, use_b = false;  // operands that are wires
    switch (in.op) {
      case WP_CONST:
        if (in.a >= p.n_consts) return wp_fail(err, "instruction %u: constant index %u is not below n_consts = %u", i, in.a, p.n_consts);
        if (in.b) return wp_fail(err, "instruction %u: operand b = %u of an instruction that has none", i, in.b);
        break;
      case WP_ADD: case WP_SUB: case WP_MUL: use_a = use_b = true; break;
      case WP_INV0:
        use_a = true;
        if (in.b) return wp_fail(err, "instruction %u: operand b = %u of an instruction that has none", i, in.b);
        break;
      case WP_BIT:
        use_a = true;
        if (in.b >= WPROG_BITS) return wp_fail(err, "instruction %u: bit index %u is not below %u", i, in.b, WPROG_BITS);
        break;
      case WP_ASSERT_ZERO:
        use_a = true;
        if (in.b >= p.n_statements) return wp_fail(err, "instruction %u: statement %u is not below n_statements = %u", i, in.b, p.n_statements);
        break;
      default: return wp_fail(err, "instruction %u: opcode %u is unknown", i, in.op);
    }
    if (use_a && in.a >= wire) return wp_fail(err, "instruction %u: operand a = %u is not a wire before wire %u", i, in.a, wire);
    if (use_b && in.b >= wire) return wp_fail(err, "instruction %u: operand b = %u is not a wire before wire %u", i, in.b, wire);
    if (in.c) return wp_fail(err, "instruction %u: operand c = %u of an instruction that has none", i, in.c);
    p.ins[i] = in;
    if (in.op != WP_ASSERT_ZERO) wire++;
  }
  p.n_wires = wire;
  p.map.resize(p.n_vars);
  for (uint32_t s = 0; s < p.n_vars; s++, q += 4) {
    p.map[s] = wp_le32(q);
    if (p.map[s] >= p.n_wires) return wp_fail(err, "signal map entry %u = %u is not below the wire count %u", s, p.map[s], p.n_wires);
  }
  if (p.map[0] != 0) return wp_fail(err, "signal map entry 0 is wire %u, not wire 0", p.map[0]);
  return true;
}

// The host twin of the two kernels: one instance through wp_begin / wp_exec, then the layout.  inputs_std: n_inputs x 32 B;
// witness_out: n_vars x 32 B (all zero unless *code == 0); wires_out (may be null): n_wires x 32 B, standard form (all zero for code 1).
inline void wprog_run_host(const WpProgram &p, const uint8_t *inputs_std, uint8_t *witness_out, uint8_t *wires_out, uint32_t *code, uint32_t *stmt) {
  std::vector<Fr> store(p.n_wires, Fr::zero()), in(p.n_inputs);
  if (p.n_inputs) memcpy(in.data(), inputs_std, (size_t)32 * p.n_inputs);
  WpLane L;
  L.store = store.data();
  L.stride = 1;
  L.consts = p.consts.data();
  const bool ran = wp_begin(L, in.data(), p.n_inputs);
  if (ran)
    for (uint32_t i = 0; i < p.n_instr; i++) wp_exec(L, p.ins[i]);
  *code = L.code;
  *stmt = L.stmt;
  memset(witness_out, 0, (size_t)32 * p.n_vars);
  if (L.code == WP_OK)
    for (uint32_t s = 0; s < p.n_vars; s++) {
      const Fr v = from_mont(store[p.map[s]]);
      memcpy(witness_out + (size_t)32 * s, v.v, 32);
    }
  if (wires_out) {
    memset(wires_out, 0, (size_t)32 * p.n_wires);
    if (ran)
      for (uint32_t w = 0; w < p.n_wires; w++) {
        const Fr v = from_mont(store[w]);
        memcpy(wires_out + (size_t)32 * w, v.v, 32);
      }
  }
}
}  // namespace zkr
