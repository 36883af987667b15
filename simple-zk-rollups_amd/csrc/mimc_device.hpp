// mimc_device.hpp -- MiMCSponge-220 for one GPU thread per hash, shared by the translation units that hash on the device
// (rollup_gpu.hip: the batch hash and the tree build; zkr_sequencer.hip: signatures, leaves and the versioned tree levels;
// zkr_book.hip: hashPair of public keys).
// The permutation of /root/reference/operator/src/utils/crypto.ts:28-38 `multiHash` (prover/circuits/hasher.circom:3-30): 220
// rounds of x -> x^5 in Fr Montgomery arithmetic, key 0.  The sponge is written once (mimc_absorb) and entered two ways that must
// stay two: mimc_hash_std takes operands of any size mod r, mimc_hash_pair takes two values known to be below r with the plain
// to_mont -- up to five compare-and-subtract rounds per operand cheaper, wrong for anything else.  The round constants live in
// __constant__ memory, one copy per translation unit that includes this header (no relocatable device code in this build);
// upload_mimc_constants fills this unit's copy once per device.
#pragma once
#include <mutex>
#include "zkr_internal.hpp"
#include "rollup_witness.hpp"

namespace zkr {
const Fr *mimc_round_constants();  // rollup.cpp

static __constant__ uint32_t c_mimc[MIMC_ROUNDS * 8];

__device__ __forceinline__ Fr mimc_const(int i) {
  Fr k;
#pragma unroll
  for (int j = 0; j < 8; j++) k.v[j] = c_mimc[8 * i + j];
  return k;
}
__device__ __forceinline__ void mimc_feistel(Fr &xl, Fr &xr) {  // key 0 (hasher.circom:21)
  for (int i = 0; i < MIMC_ROUNDS; i++) {
    Fr t = add(xl, mimc_const(i));
    Fr t2 = sqr(t);
    Fr t5 = mul(sqr(t2), t);
    if (i < MIMC_ROUNDS - 1) {
      Fr nl = add(xr, t5);
      xr = xl;
      xl = nl;
    } else {
      xr = add(xr, t5);
    }
  }
}
__device__ __forceinline__ Fr load_std_as_mont(const Fr *p) {
  Fr a = *p;
  // operands of any size are taken mod r as the reference's field operations do: 2^256 < 6 r
  for (int k = 0; k < 5; k++) {
    bool ge = true;
    for (int i = 7; i >= 0; i--)
      if (a.v[i] != FrParams::P[i]) { ge = a.v[i] > FrParams::P[i]; break; }
    if (!ge) break;
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) a.v[i] = __builtin_subc(a.v[i], FrParams::P[i], br, &br);
  }
  return to_mont(a);
}
// The sponge (crypto.ts:28-34): r += x, then the permutation.  r, c and x are Montgomery; a hash starts from r = c = 0.
__device__ __forceinline__ void mimc_absorb(Fr &r, Fr &c, const Fr &x) {
  r = add(r, x);
  mimc_feistel(r, c);
}
// multiHash of n standard-form elements of ANY size, each taken mod r: leaves, messages, the batch hash.  Montgomery out.
__device__ __forceinline__ Fr mimc_hash_std(const Fr *in, uint32_t n) {
  Fr r = Fr::zero(), c = Fr::zero();
  for (uint32_t i = 0; i < n; i++) mimc_absorb(r, c, load_std_as_mont(in + i));
  return r;
}
// hashLeftRight (crypto.ts:36-38) of two standard-form values KNOWN to be below r (nodes, hashes, checked keys); standard form out
__device__ __forceinline__ Fr mimc_hash_pair(const Fr &left, const Fr &right) {
  Fr r = to_mont(left), c = Fr::zero();
  mimc_feistel(r, c);
  mimc_absorb(r, c, to_mont(right));
  return from_mont(r);
}

static int upload_mimc_constants(int device) {
  static std::mutex mu;
  static bool done[64] = {false};
  std::lock_guard<std::mutex> lk(mu);
  if (device < 64 && done[device]) return 0;
  ZKR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_mimc), mimc_round_constants(), MIMC_ROUNDS * 32));
  if (device < 64) done[device] = true;
  return 0;
}
}  // namespace zkr
