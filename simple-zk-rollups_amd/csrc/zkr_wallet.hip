// zkr_wallet.hip -- the user's side of the reference's operator/src/utils/crypto.ts and the reference's second circuit in bulk on the
// GPU: formatPrivKeyForBabyJub (:58-76), genPublicKey (:78-84) and sign (:143-168) for many keys, and
// `Circuit.calculateWitness` for withdraw.circom (operator/src/snarks/withdraw.ts:6-10) for many withdrawals, left in device memory
// for zkr_prove_batch_device.  The programs are wallet_program.hpp's, the same text the host hooks below run: one thread per item,
// each a chain of dependent products over Fr (MiMCSponge-220 permutations, 253-step fixed-base chains over the table 2^i BASE8
// the transaction witness builder uploaded: rollup_gpu.hip rollup_device_tables), so these are latency chains like
// seq_verify_kernel and rollup_witness_tx_kernel, 64 threads to a block.  NOT constant time.
// Everything that held a key, a formatted scalar or a partial sum of key * BASE8 on the device is zeroed before it is freed; a
// nonce r lives in registers only.  The host side stages nothing: keys are copied from the caller's memory.
#include <string.h>
#include <vector>
#include "zkr_internal.hpp"
#include "wallet_program.hpp"

namespace zkr {
int rollup_device_tables(int device, TxConsts *k);                                               // rollup_gpu.hip

// out[t] = formatPrivKeyForBabyJub(privs[t])
static __global__ __launch_bounds__(64) void wallet_format_kernel(const Fr *privs, size_t n, TxConsts k, Fr *out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fr p;
  wl_read(privs + t, p);
  uint32_t f[8];
  wl_format_privkey(k, p, f);
  Fr o;
#pragma unroll
  for (int i = 0; i < 8; i++) o.v[i] = f[i];
  out[t] = o;
}
// pubs[2t], pubs[2t + 1] = genPublicKey(privs[t])
static __global__ __launch_bounds__(64) void wallet_pubkey_kernel(const Fr *privs, size_t n, TxConsts k, Fr *pubs) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fr p, ax, ay;
  wl_read(privs + t, p);
  uint32_t f[8];
  wl_format_privkey(k, p, f);
  wl_pubkey(k, f, ax, ay);
  pubs[2 * t] = from_mont(ax), pubs[2 * t + 1] = from_mont(ay);
}
// sigs[3t ..] = sign(privs[t], msgs[t * arity ..]): R8x R8y S
static __global__ __launch_bounds__(64) void wallet_sign_kernel(const Fr *privs, const Fr *msgs, uint32_t arity, size_t n, TxConsts k, Fr *sigs) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fr p, r8x, r8y, s;
  wl_read(privs + t, p);
  uint32_t S[8];
  wl_sign(k, p, msgs + t * arity, arity, r8x, r8y, S);
#pragma unroll
  for (int i = 0; i < 8; i++) s.v[i] = S[i];
  sigs[3 * t] = from_mont(r8x), sigs[3 * t + 1] = from_mont(r8y), sigs[3 * t + 2] = s;
}
// One thread per withdrawal.  in: n keys, then n nullifiers (standard form); wit: n x WD_NVARS -- a thread writes its private
// signals (Montgomery for now) behind the five leading signals of its witness and its public key into signals 1, 2.
static __global__ __launch_bounds__(64) void withdraw_witness_kernel(const Fr *in, uint32_t n, TxConsts k, Fr *wit, Fr *workspace, uint32_t *errs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fr *w = wit + (size_t)t * WD_NVARS;
  errs[t] = wd_witness(k, in + t, in + n + t, w + WD_PUBLIC, workspace + (size_t)t * WD_WS_ELEMS, w + 1);
}
// The vector as binarifyWitness lays it out: signal 0 = 1, the nullifier and the key as given, everything else to standard form
// in place.  Thread per signal of every witness.
static __global__ __launch_bounds__(256) void withdraw_layout_kernel(const Fr *in, uint32_t n, Fr *wit) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)n * WD_NVARS) return;
  const size_t t = g / WD_NVARS;
  const uint32_t s = (uint32_t)(g % WD_NVARS);
  Fr v;
  if (s == 0) {
    v = Fr::zero();
    v.v[0] = 1;
  } else if (s == 3) {
    v = in[n + t];
  } else if (s == 4) {
    v = in[t];
  } else {
    v = from_mont(wit[g]);
  }
  wit[g] = v;
}

// index of the first of `count` elements (32 B, standard form) that is not below r, or `count`
static size_t first_not_below_r(const uint8_t *p, size_t count) {
  for (size_t i = 0; i < count; i++) {
    uint32_t w[8];
    memcpy(w, p + 32 * i, 32);
    if (!words_below(w, FrParams::P)) return i;
  }
  return count;
}
enum : size_t { WALLET_PIECE = (size_t)1 << 20, WITHDRAW_PIECE = 4096 };  // items per launch: 32 MB of keys; 128 MB of chain workspace

enum WalletOp { OP_FORMAT, OP_PUBKEY, OP_SIGN };
// The three calls over keys: checks, then the device, then piece by piece upload, kernel, results back.
static int wallet_batch(WalletOp op, const uint8_t *privs, const uint8_t *msgs, unsigned arity, size_t n, uint8_t *out, int device, const char *what) {
  if (n && (!privs || !out || (op == OP_SIGN && !msgs))) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (op == OP_SIGN && (arity < 1 || arity > 64)) { set_error("message arity %u out of range (1..64)", arity); return ZKR_ERR_ARG; }
  {
    const size_t bad = first_not_below_r(privs, n);
    if (bad < n) { set_error("item %zu: private key >= r", bad); return ZKR_ERR_ARG; }
    if (op == OP_SIGN) {
      const size_t badm = first_not_below_r(msgs, n * arity);
      if (badm < n * arity) { set_error("item %zu: message element %zu >= r", badm / arity, badm % arity); return ZKR_ERR_ARG; }
    }
  }
  if (n == 0) return ZKR_OK;
  int rc = need_device(device, what);
  if (rc) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  TxConsts k;
  if ((rc = rollup_device_tables(device, &k))) return rc;
  const size_t out_per = op == OP_FORMAT ? 1 : op == OP_PUBKEY ? 2 : 3, piece = n < WALLET_PIECE ? n : WALLET_PIECE;
  SecretBuf d_priv, d_out;  // the formatted scalars are secrets too
  DevBuf d_msgs;
  if ((rc = d_priv.alloc(piece * 32)) || (rc = d_out.alloc(piece * out_per * 32))) return rc;
  if (op == OP_SIGN && (rc = d_msgs.alloc(piece * arity * 32))) return rc;
  for (size_t at = 0; at < n; at += piece) {
    const size_t cnt = n - at < piece ? n - at : piece;
    ZKR_HIP_CHECK(hipMemcpy(d_priv.p, privs + at * 32, cnt * 32, hipMemcpyHostToDevice));
    if (op == OP_SIGN) ZKR_HIP_CHECK(hipMemcpy(d_msgs.p, msgs + at * arity * 32, cnt * arity * 32, hipMemcpyHostToDevice));
    if (op == OP_FORMAT) wallet_format_kernel<<<blocks_of(cnt, 64), 64>>>(d_priv.as<Fr>(), cnt, k, d_out.as<Fr>());
    else if (op == OP_PUBKEY) wallet_pubkey_kernel<<<blocks_of(cnt, 64), 64>>>(d_priv.as<Fr>(), cnt, k, d_out.as<Fr>());
    else wallet_sign_kernel<<<blocks_of(cnt, 64), 64>>>(d_priv.as<Fr>(), d_msgs.as<Fr>(), arity, cnt, k, d_out.as<Fr>());
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpy(out + at * out_per * 32, d_out.p, cnt * out_per * 32, hipMemcpyDeviceToHost));
  }
  return ZKR_OK;
}
}  // namespace zkr

using namespace zkr;

extern "C" {

int zkr_babyjub_format_privkey_batch(const uint8_t *privs, size_t n, uint8_t *out, int device) {
  return wallet_batch(OP_FORMAT, privs, nullptr, 0, n, out, device, "the batch key formatting (zkr_babyjub_format_privkey is the host call)");
}
int zkr_babyjub_pubkey_batch(const uint8_t *privs, size_t n, uint8_t *pubs, int device) {
  return wallet_batch(OP_PUBKEY, privs, nullptr, 0, n, pubs, device, "the batch key derivation (zkr_babyjub_pubkey is the host call)");
}
int zkr_eddsa_sign_batch(const uint8_t *privs, const uint8_t *msgs, unsigned arity, size_t n, uint8_t *sigs, int device) {
  return wallet_batch(OP_SIGN, privs, msgs, arity, n, sigs, device, "the batch signer (zkr_eddsa_sign is the host call)");
}

int zkr_withdraw_witness_batch_device(const uint8_t *private_keys, const uint8_t *nullifiers, size_t n, void *d_witnesses, int device, void *stream) {
  if (n && (!private_keys || !nullifiers || !d_witnesses)) { set_error("null argument"); return ZKR_ERR_ARG; }
  {
    const size_t badk = first_not_below_r(private_keys, n), badn = first_not_below_r(nullifiers, n);
    if (badk < n || badn < n) { set_error("witness %zu: input >= r", badk < badn ? badk : badn); return ZKR_ERR_ARG; }
  }
  if (n == 0) return ZKR_OK;
  int rc = need_device(device, "the batch withdraw witness builder (zkr_withdraw_witness is the host call)");
  if (rc) return rc;
  for (size_t i = 0; i < n; i++)  // the program's first statement (wd_witness: nothing above the 253 bit signals), before any output is written
    if (private_keys[32 * i + 31] >> 5) { set_error("witness %zu violates: %s", i, wd_statement_text(WD_KEY_BITS)); return ZKR_ERR_UNSATISFIED; }
  ZKR_HIP_CHECK(hipSetDevice(device));
  TxConsts k;
  if ((rc = rollup_device_tables(device, &k))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t piece = n < WITHDRAW_PIECE ? n : WITHDRAW_PIECE;
  SecretBuf d_in, d_ws;
  d_in.s = d_ws.s = s;
  DevBuf d_errs;
  if ((rc = d_in.alloc(2 * piece * 32)) || (rc = d_ws.alloc(piece * WD_WS_ELEMS * 32)) || (rc = d_errs.alloc(piece * 4))) return rc;
  std::vector<uint32_t> errs(piece);
  for (size_t at = 0; at < n; at += piece) {
    const size_t cnt = n - at < piece ? n - at : piece;
    Fr *wit = (Fr *)d_witnesses + at * WD_NVARS;
    ZKR_HIP_CHECK(hipMemcpyAsync(d_in.p, private_keys + at * 32, cnt * 32, hipMemcpyHostToDevice, s));
    ZKR_HIP_CHECK(hipMemcpyAsync(d_in.as<Fr>() + cnt, nullifiers + at * 32, cnt * 32, hipMemcpyHostToDevice, s));
    withdraw_witness_kernel<<<blocks_of(cnt, 64), 64, 0, s>>>(d_in.as<Fr>(), (uint32_t)cnt, k, wit, d_ws.as<Fr>(), d_errs.as<uint32_t>());
    ZKR_HIP_CHECK(hipGetLastError());
    withdraw_layout_kernel<<<blocks_of(cnt * WD_NVARS, 256), 256, 0, s>>>(d_in.as<Fr>(), (uint32_t)cnt, wit);
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpyAsync(errs.data(), d_errs.p, cnt * 4, hipMemcpyDeviceToHost, s));
    ZKR_HIP_CHECK(hipStreamSynchronize(s));
    for (size_t i = 0; i < cnt; i++) {
      const uint32_t e = errs[i];
      if (e == ST_INPUT_RANGE) { set_error("witness %zu: input >= r", at + i); return ZKR_ERR_ARG; }
      if (e == ST_COUNT) { set_error("internal: private signal count differs from the withdraw circuit's"); return ZKR_ERR_HIP; }
      if (e) { set_error("witness %zu violates: %s", at + i, wd_statement_text(e)); return ZKR_ERR_UNSATISFIED; }
    }
  }
  return ZKR_OK;
}

// ---- test hooks: the same programs on the host, one item
int zkr_wallet_pubkey_program_host(const uint8_t priv[32], uint8_t formatted[32], uint8_t pub[64]) {
  if (!priv || !formatted || !pub) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (first_not_below_r(priv, 1) < 1) { set_error("private key >= r"); return ZKR_ERR_ARG; }
  std::vector<Fr> tab;
  TxConsts k;
  wl_host_tables(tab, k);
  Fr ps, p, ax, ay;
  memcpy(ps.v, priv, 32);
  wl_read(&ps, p);
  uint32_t f[8];
  wl_format_privkey(k, p, f);
  memcpy(formatted, f, 32);
  wl_pubkey(k, f, ax, ay);
  ax = from_mont(ax), ay = from_mont(ay);
  memcpy(pub, ax.v, 32);
  memcpy(pub + 32, ay.v, 32);
  return ZKR_OK;
}
int zkr_wallet_sign_program_host(const uint8_t priv[32], const uint8_t *msg, unsigned arity, uint8_t sig[96]) {
  if (!priv || !msg || !sig) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (arity < 1 || arity > 64) { set_error("message arity %u out of range (1..64)", arity); return ZKR_ERR_ARG; }
  if (first_not_below_r(priv, 1) < 1) { set_error("private key >= r"); return ZKR_ERR_ARG; }
  {
    const size_t bad = first_not_below_r(msg, arity);
    if (bad < arity) { set_error("message element %zu >= r", bad); return ZKR_ERR_ARG; }
  }
  std::vector<Fr> tab, m(arity);
  TxConsts k;
  wl_host_tables(tab, k);
  memcpy(m.data(), msg, (size_t)arity * 32);
  Fr ps, p, r8x, r8y;
  memcpy(ps.v, priv, 32);
  wl_read(&ps, p);
  uint32_t S[8];
  wl_sign(k, p, m.data(), arity, r8x, r8y, S);
  r8x = from_mont(r8x), r8y = from_mont(r8y);
  memcpy(sig, r8x.v, 32);
  memcpy(sig + 32, r8y.v, 32);
  memcpy(sig + 64, S, 32);
  return ZKR_OK;
}
int zkr_withdraw_witness_program_host(const uint8_t private_key[32], const uint8_t nullifier[32], uint8_t *witness_out, uint32_t *stmt) {
  if (!private_key || !nullifier || !witness_out || !stmt) { set_error("null argument"); return ZKR_ERR_ARG; }
  std::vector<Fr> tab, w(WD_NVARS), ws(WD_WS_ELEMS);
  TxConsts k;
  wl_host_tables(tab, k);
  Fr key, nul;
  memcpy(key.v, private_key, 32);
  memcpy(nul.v, nullifier, 32);
  *stmt = wd_witness(k, &key, &nul, w.data() + WD_PUBLIC, ws.data(), w.data() + 1);
  if (*stmt == ST_INPUT_RANGE) { set_error("input >= r"); return ZKR_ERR_ARG; }
  if (*stmt) return ZKR_OK;
  Fr *out = reinterpret_cast<Fr *>(witness_out);
  for (uint32_t s = 0; s < WD_NVARS; s++) out[s] = from_mont(w[s]);
  Fr one = Fr::zero();
  one.v[0] = 1;
  out[0] = one, out[3] = nul, out[4] = key;
  return ZKR_OK;
}
const char *zkr_withdraw_statement_text(uint32_t stmt) { return wd_statement_text(stmt); }
uint32_t zkr_withdraw_n_vars(void) { return WD_NVARS; }

}  // extern "C"
