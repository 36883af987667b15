// zkr_crypto.hip -- the rest of the reference's operator/src/utils/crypto.ts: ecdh (:86-93), encrypt (:95-110), decrypt (:112-123)
// and their compositions ecdhEncrypt / ecdhDecrypt (:125-141), one item on the host and whole lists on the GPU.
// The programs are crypto_program.hpp's, the same text for the host calls and the kernels.
//   ecdh_kernel     one lane per (private key, public key): format the key, 253 doublings and additions, one inversion
//   iv_kernel       one lane per message: multiHash(msg, 0) is a sequential sponge over the message's elements
//   cipher_kernel   one lane per ELEMENT of the flat n x arity grid: element i of message t takes hash(key_t, iv_t + i), and all
//                   of them are independent, so a long message fills the device as well as many short ones do.  The lanes of
//                   a wavefront may belong to different messages; all of them are in the same round of the same hash.
// Every kernel is a chain of dependent products over Fr, 64 threads to a block like the wallet kernels; no LDS, no barrier.
// The MiMC7 round constants live in __constant__ memory, filled once per device.  NOT constant time.
// Everything that held a private key, a shared key, a cipher key or a plaintext on the device is zeroed before it is freed; in
// the ecdh* calls the shared keys never leave the device.
#include <string.h>
#include <mutex>
#include <vector>
#include "zkr_internal.hpp"
#include "crypto_program.hpp"

namespace zkr {
const Fr *mimc7_round_constants();                                                               // rollup.cpp
int rollup_device_tables(int device, TxConsts *k);                                               // rollup_gpu.hip

static __constant__ uint32_t c_mimc7[MIMC7_ROUNDS * 8];
struct Mimc7ConstDev {
  __device__ __forceinline__ Fr operator()(int i) const {
    Fr k;
#pragma unroll
    for (int j = 0; j < 8; j++) k.v[j] = c_mimc7[8 * i + j];
    return k;
  }
};
static int upload_mimc7_constants(int device) {
  static std::mutex mu;
  static bool done[64] = {false};
  std::lock_guard<std::mutex> lk(mu);
  if (device < 64 && done[device]) return 0;
  ZKR_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_mimc7), mimc7_round_constants(), MIMC7_ROUNDS * 32));
  if (device < 64) done[device] = true;
  return 0;
}

// a 32-byte element as two 16-byte accesses (the buffers are hipMalloc's, the elements 32 bytes apart)
__device__ __forceinline__ Fr load_elem(const Fr *p) {
  const uint4 lo = reinterpret_cast<const uint4 *>(p)[0], hi = reinterpret_cast<const uint4 *>(p)[1];
  Fr a;
  a.v[0] = lo.x, a.v[1] = lo.y, a.v[2] = lo.z, a.v[3] = lo.w, a.v[4] = hi.x, a.v[5] = hi.y, a.v[6] = hi.z, a.v[7] = hi.w;
  return a;
}
__device__ __forceinline__ void store_elem(Fr *p, const Fr &a) {
  reinterpret_cast<uint4 *>(p)[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  reinterpret_cast<uint4 *>(p)[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}

// shared[t] = ecdh(privs[t], pubs[2t], pubs[2t + 1]); everything standard form and checked by the host
static __global__ __launch_bounds__(64) void ecdh_kernel(const Fr *privs, const Fr *pubs, uint32_t n, TxConsts k, Fr *shared) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Fr p = to_mont(load_elem(privs + t)), px = to_mont(load_elem(pubs + 2 * (size_t)t)), py = to_mont(load_elem(pubs + 2 * (size_t)t + 1));
  store_elem(shared + t, from_mont(cr_ecdh(k, p, px, py)));
}
// ivs[t] = multiHash(msgs[t * arity ..], 0)
static __global__ __launch_bounds__(64) void iv_kernel(const Fr *msgs, uint32_t arity, uint32_t n, Fr *ivs) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Mimc7ConstDev c;
  const Fr *m = msgs + (size_t)t * arity;
  Fr r = Fr::zero();
#pragma unroll 1
  for (uint32_t i = 0; i < arity; i++) r = cr_mimc7_absorb(c, r, to_mont(load_elem(m + i)));
  store_elem(ivs + t, from_mont(r));
}
// out[g] = in[g] (+ or -) hash(keys[t], ivs[t] + i) for element g = t * arity + i of the flat grid; total = n * arity < 2^32
template <bool DECRYPT>
static __global__ __launch_bounds__(64) void cipher_kernel(const Fr *keys, const Fr *ivs, const Fr *in, uint32_t arity, uint32_t total, Fr *out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const uint32_t t = g / arity, i = g - t * arity;
  const Mimc7ConstDev c;
  const Fr ks = cr_keystream(c, to_mont(load_elem(keys + t)), to_mont(load_elem(ivs + t)), i);
  const Fr e = load_elem(in + g);
  store_elem(out + g, DECRYPT ? cr_decrypt_element(e, ks) : cr_encrypt_element(e, ks));
}

static Fr read_words(const uint8_t *p) {
  Fr a;
  memcpy(a.v, p, 32);
  return a;
}
static bool below_r(const uint8_t *p) { return words_below(read_words(p).v, FrParams::P); }

// What a call is given; a null pointer stands for "this call has no such argument".
struct CryptoIn {
  const char *key_name = "key";  // "private key" where the keys are those of ecdh
  const uint8_t *keys = nullptr;  // n x 32 B
  const uint8_t *pubs = nullptr;  // n x 64 B
  const uint8_t *ivs = nullptr;   // n x 32 B (decrypt)
  const uint8_t *elems = nullptr;  // n x arity x 32 B: plaintext, or ciphertext where ivs is set
  unsigned arity = 0;
  size_t n = 0;
};
// The refusals, item by item and in the order key, public key, iv, elements; they name the first offending item.  No device.
static int crypto_check(const CryptoIn &in) {
  TxConsts k;
  std::vector<Fr> tab;
  if (in.pubs && in.n) wl_host_tables(tab, k);
  for (size_t t = 0; t < in.n; t++) {
    if (!below_r(in.keys + 32 * t)) { set_error("item %zu: %s >= r", t, in.key_name); return ZKR_ERR_ARG; }
    if (in.pubs) {
      for (int j = 0; j < 2; j++)
        if (!below_r(in.pubs + 64 * t + 32 * j)) { set_error("item %zu: public key coordinate %d >= r", t, j); return ZKR_ERR_ARG; }
      if (!bj_on_curve(k.a, k.d, to_mont(read_words(in.pubs + 64 * t)), to_mont(read_words(in.pubs + 64 * t + 32)))) {
        set_error("item %zu: public key is not on the curve", t);
        return ZKR_ERR_ARG;
      }
    }
    if (in.ivs && !below_r(in.ivs + 32 * t)) { set_error("item %zu: iv >= r", t); return ZKR_ERR_ARG; }
    for (size_t i = 0; in.elems && i < in.arity; i++) {
      const uint8_t *e = in.elems + 32 * (t * in.arity + i);
      if (in.ivs) {
        if (!cr_below_2r(read_words(e))) { set_error("item %zu: ciphertext element %zu >= 2r", t, i); return ZKR_ERR_ARG; }
      } else if (!below_r(e)) {
        set_error("item %zu: message element %zu >= r", t, i);
        return ZKR_ERR_ARG;
      }
    }
  }
  return ZKR_OK;
}
static int check_arity(unsigned arity) {
  if (arity < 1 || arity > CRYPTO_MAX_ARITY) { set_error("message arity %u out of range (1..%u)", arity, CRYPTO_MAX_ARITY); return ZKR_ERR_ARG; }
  return ZKR_OK;
}

enum : size_t { ECDH_PIECE = (size_t)1 << 20, CIPHER_PIECE_ELEMS = (size_t)1 << 22 };  // per launch: 32 MB of keys; 128 MB of elements

// The batch calls: checks, then the device, then piece by piece upload, kernels on one stream, results back.
//   ecdh: the keys are private keys and the cipher keys are the shared keys, which stay on the device unless they are the result
//   (CR_SHARED: shared_out).  The callers have refused null pointers.
enum CryptoOp { CR_SHARED, CR_ENCRYPT, CR_DECRYPT };
static int crypto_batch(CryptoOp op, bool ecdh, const CryptoIn &in, uint8_t *shared_out, uint8_t *ivs_out, uint8_t *out, int device, const char *what) {
  const bool cipher = op != CR_SHARED, decrypt = op == CR_DECRYPT;
  const size_t n = in.n;
  int rc;
  if (cipher && (rc = check_arity(in.arity))) return rc;
  if ((rc = crypto_check(in))) return rc;
  if (n == 0) return ZKR_OK;
  if ((rc = need_device(device, what))) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  TxConsts k;
  if (ecdh && (rc = rollup_device_tables(device, &k))) return rc;
  if (cipher && (rc = upload_mimc7_constants(device))) return rc;
  const size_t arity = in.arity;
  size_t piece = cipher ? CIPHER_PIECE_ELEMS / arity : ECDH_PIECE;
  if (piece < 1) piece = 1;
  if (piece > n) piece = n;
  SecretBuf d_keys, d_shared, d_in, d_out;  // plaintexts are secrets as the keys are
  DevBuf d_pubs, d_ivs;
  if ((rc = d_keys.alloc(piece * 32))) return rc;
  if (ecdh && ((rc = d_pubs.alloc(piece * 64)) || (rc = d_shared.alloc(piece * 32)))) return rc;
  if (cipher && ((rc = d_ivs.alloc(piece * 32)) || (rc = d_in.alloc(piece * arity * 32)) || (rc = d_out.alloc(piece * arity * 32)))) return rc;
  for (size_t at = 0; at < n; at += piece) {
    const size_t cnt = n - at < piece ? n - at : piece;
    ZKR_HIP_CHECK(hipMemcpy(d_keys.p, in.keys + at * 32, cnt * 32, hipMemcpyHostToDevice));
    const Fr *keys = d_keys.as<Fr>();
    if (ecdh) {
      ZKR_HIP_CHECK(hipMemcpy(d_pubs.p, in.pubs + at * 64, cnt * 64, hipMemcpyHostToDevice));
      ecdh_kernel<<<blocks_of(cnt, 64), 64>>>(d_keys.as<Fr>(), d_pubs.as<Fr>(), (uint32_t)cnt, k, d_shared.as<Fr>());
      ZKR_HIP_CHECK(hipGetLastError());
      keys = d_shared.as<Fr>();
    }
    if (!cipher) {
      ZKR_HIP_CHECK(hipMemcpy(shared_out + at * 32, d_shared.p, cnt * 32, hipMemcpyDeviceToHost));
      continue;
    }
    const size_t total = cnt * arity;  // <= max(2^22, 65536)
    ZKR_HIP_CHECK(hipMemcpy(d_in.p, in.elems + at * arity * 32, total * 32, hipMemcpyHostToDevice));
    if (decrypt) {
      ZKR_HIP_CHECK(hipMemcpy(d_ivs.p, in.ivs + at * 32, cnt * 32, hipMemcpyHostToDevice));
      cipher_kernel<true><<<blocks_of(total, 64), 64>>>(keys, d_ivs.as<Fr>(), d_in.as<Fr>(), (uint32_t)arity, (uint32_t)total, d_out.as<Fr>());
    } else {
      iv_kernel<<<blocks_of(cnt, 64), 64>>>(d_in.as<Fr>(), (uint32_t)arity, (uint32_t)cnt, d_ivs.as<Fr>());
      ZKR_HIP_CHECK(hipGetLastError());
      cipher_kernel<false><<<blocks_of(total, 64), 64>>>(keys, d_ivs.as<Fr>(), d_in.as<Fr>(), (uint32_t)arity, (uint32_t)total, d_out.as<Fr>());
    }
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpy(out + at * arity * 32, d_out.p, total * 32, hipMemcpyDeviceToHost));
    if (!decrypt) ZKR_HIP_CHECK(hipMemcpy(ivs_out + at * 32, d_ivs.p, cnt * 32, hipMemcpyDeviceToHost));
  }
  return ZKR_OK;
}
}  // namespace zkr

using namespace zkr;

extern "C" {

// ---- one item on the host
int zkr_mimc7_round_constants(uint8_t *out) {
  if (!out) { set_error("null argument"); return ZKR_ERR_ARG; }
  const Fr *c = mimc7_round_constants();
  for (int i = 0; i < MIMC7_ROUNDS; i++) {
    const Fr s = from_mont(c[i]);
    memcpy(out + 32 * i, s.v, 32);
  }
  return ZKR_OK;
}
int zkr_mimc7_hash(const uint8_t x[32], const uint8_t k[32], uint8_t out[32]) {
  if (!x || !k || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (!below_r(x)) { set_error("x >= r"); return ZKR_ERR_ARG; }
  if (!below_r(k)) { set_error("key >= r"); return ZKR_ERR_ARG; }
  const Fr h = from_mont(cr_mimc7_hash(Mimc7ConstPtr{mimc7_round_constants()}, to_mont(read_words(x)), to_mont(read_words(k))));
  memcpy(out, h.v, 32);
  return ZKR_OK;
}
int zkr_mimc7_multihash(const uint8_t *in, size_t n, const uint8_t key[32], uint8_t out[32]) {
  if ((!in && n) || !key || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (!below_r(key)) { set_error("key >= r"); return ZKR_ERR_ARG; }
  const Mimc7ConstPtr c{mimc7_round_constants()};
  Fr r = to_mont(read_words(key));
  for (size_t i = 0; i < n; i++) {
    if (!below_r(in + 32 * i)) { set_error("element %zu >= r", i); return ZKR_ERR_ARG; }
    r = cr_mimc7_absorb(c, r, to_mont(read_words(in + 32 * i)));
  }
  r = from_mont(r);
  memcpy(out, r.v, 32);
  return ZKR_OK;
}
int zkr_babyjub_ecdh(const uint8_t priv[32], const uint8_t pub[64], uint8_t shared[32]) {
  if (!priv || !pub || !shared) { set_error("null argument"); return ZKR_ERR_ARG; }
  CryptoIn in;
  in.key_name = "private key", in.keys = priv, in.pubs = pub, in.n = 1;
  if (int rc = crypto_check(in)) return rc;
  std::vector<Fr> tab;
  TxConsts k;
  wl_host_tables(tab, k);
  const Fr s = from_mont(cr_ecdh(k, to_mont(read_words(priv)), to_mont(read_words(pub)), to_mont(read_words(pub + 32))));
  memcpy(shared, s.v, 32);
  return ZKR_OK;
}
int zkr_mimc7_encrypt(const uint8_t key[32], const uint8_t *msg, unsigned arity, uint8_t iv[32], uint8_t *out) {
  if (!key || !msg || !iv || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = check_arity(arity)) return rc;
  CryptoIn in;
  in.keys = key, in.elems = msg, in.arity = arity, in.n = 1;
  if (int rc = crypto_check(in)) return rc;
  const Mimc7ConstPtr c{mimc7_round_constants()};
  std::vector<Fr> m(arity);
  memcpy(m.data(), msg, (size_t)arity * 32);
  const Fr km = to_mont(read_words(key)), ivm = cr_mimc7_multihash(c, m.data(), arity, Fr::zero());
  for (unsigned i = 0; i < arity; i++) {
    const Fr e = cr_encrypt_element(m[i], cr_keystream(c, km, ivm, i));
    memcpy(out + 32 * (size_t)i, e.v, 32);
  }
  const Fr ivs = from_mont(ivm);
  memcpy(iv, ivs.v, 32);
  return ZKR_OK;
}
int zkr_mimc7_decrypt(const uint8_t key[32], const uint8_t iv[32], const uint8_t *enc, unsigned arity, uint8_t *out) {
  if (!key || !iv || !enc || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (int rc = check_arity(arity)) return rc;
  CryptoIn in;
  in.keys = key, in.ivs = iv, in.elems = enc, in.arity = arity, in.n = 1;
  if (int rc = crypto_check(in)) return rc;
  const Mimc7ConstPtr c{mimc7_round_constants()};
  const Fr km = to_mont(read_words(key)), ivm = to_mont(read_words(iv));
  for (unsigned i = 0; i < arity; i++) {
    const Fr e = cr_decrypt_element(read_words(enc + 32 * (size_t)i), cr_keystream(c, km, ivm, i));
    memcpy(out + 32 * (size_t)i, e.v, 32);
  }
  return ZKR_OK;
}

// ---- whole lists on the GPU
int zkr_babyjub_ecdh_batch(const uint8_t *privs, const uint8_t *pubs, size_t n, uint8_t *shared, int device) {
  if (n && (!privs || !pubs || !shared)) { set_error("null argument"); return ZKR_ERR_ARG; }
  CryptoIn in;
  in.key_name = "private key", in.keys = privs, in.pubs = pubs, in.n = n;
  return crypto_batch(CR_SHARED, true, in, shared, nullptr, nullptr, device, "the batch key agreement (zkr_babyjub_ecdh is the host call)");
}
int zkr_mimc7_encrypt_batch(const uint8_t *keys, const uint8_t *msgs, unsigned arity, size_t n, uint8_t *ivs, uint8_t *out, int device) {
  if (n && (!keys || !msgs || !ivs || !out)) { set_error("null argument"); return ZKR_ERR_ARG; }
  CryptoIn in;
  in.keys = keys, in.elems = msgs, in.arity = arity, in.n = n;
  return crypto_batch(CR_ENCRYPT, false, in, nullptr, ivs, out, device, "the batch cipher (zkr_mimc7_encrypt is the host call)");
}
int zkr_mimc7_decrypt_batch(const uint8_t *keys, const uint8_t *ivs, const uint8_t *encs, unsigned arity, size_t n, uint8_t *out, int device) {
  if (n && (!keys || !ivs || !encs || !out)) { set_error("null argument"); return ZKR_ERR_ARG; }
  CryptoIn in;
  in.keys = keys, in.ivs = ivs, in.elems = encs, in.arity = arity, in.n = n;
  return crypto_batch(CR_DECRYPT, false, in, nullptr, nullptr, out, device, "the batch cipher (zkr_mimc7_decrypt is the host call)");
}
int zkr_ecdh_encrypt_batch(const uint8_t *privs, const uint8_t *pubs, const uint8_t *msgs, unsigned arity, size_t n, uint8_t *ivs, uint8_t *out, int device) {
  if (n && (!privs || !pubs || !msgs || !ivs || !out)) { set_error("null argument"); return ZKR_ERR_ARG; }
  CryptoIn in;
  in.key_name = "private key", in.keys = privs, in.pubs = pubs, in.elems = msgs, in.arity = arity, in.n = n;
  return crypto_batch(CR_ENCRYPT, true, in, nullptr, ivs, out, device, "the batch ecdhEncrypt (zkr_babyjub_ecdh and zkr_mimc7_encrypt are the host calls)");
}
int zkr_ecdh_decrypt_batch(const uint8_t *privs, const uint8_t *pubs, const uint8_t *ivs, const uint8_t *encs, unsigned arity, size_t n, uint8_t *out, int device) {
  if (n && (!privs || !pubs || !ivs || !encs || !out)) { set_error("null argument"); return ZKR_ERR_ARG; }
  CryptoIn in;
  in.key_name = "private key", in.keys = privs, in.pubs = pubs, in.ivs = ivs, in.elems = encs, in.arity = arity, in.n = n;
  return crypto_batch(CR_DECRYPT, true, in, nullptr, nullptr, out, device, "the batch ecdhDecrypt (zkr_babyjub_ecdh and zkr_mimc7_decrypt are the host calls)");
}

}  // extern "C"
