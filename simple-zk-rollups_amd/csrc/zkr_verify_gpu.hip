// zkr_verify_gpu.hip -- the Groth16 acceptance check on the GPU, one verdict per proof (zkr_vk_load, zkr_verify_each,
// zkr_verify_each_device) and the pairing by itself (zkr_pairing_device).  The arithmetic is pairing.hpp, the same header code
// the host verifier runs (zkr_verify.hip), compiled for the device with real calls at the Fq2 product and above; the key parser
// is verify_key.hpp.  DESIGN.md "Verifying on the device" has the kernel split.
//
// Four kernels per piece of a batch, all on the 8 x 32-bit Fq of field.hpp, no LDS, no barrier, 64 lanes per workgroup:
//   ingest   one lane per proof: range, curve and subgroup checks -> Montgomery points and a verdict code;
//   vk_x     one lane per proof: IC_0 + sum_j input_j IC_{j+1} over the key's 8-bit window table;
//   miller   one lane per (proof, pair), the pair on blockIdx.y so that a wavefront runs ONE kind of loop:
//            0 = (-A, B) by projective steps, 1 = (vk_x, gamma), 2 = (C, delta) over the key's prepared lines;
//   finish   one lane per proof: f_alfa_beta * f_pub * f_proof, final exponentiation, comparison with one.
// A proof that has a verdict is skipped by the kernels behind it: its lane returns, there is nothing to wait for.
// These kernels call functions, so they have a stack in private memory (profiles/verify_device.md has the sizes): this
// translation unit is kept apart from zkr_prove / zkr_key, whose kernels are pinned to zero scratch.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "pairing.hpp"
#include "zkr_internal.hpp"
#include "verify_key.hpp"

using namespace zkr;
using pairing::Consts;
using pairing::Fq12;
using pairing::Line;

namespace zkr {

constexpr unsigned VERIFY_THREADS = 64;  // one wavefront per workgroup: a batch spreads over as many CUs as it has wavefronts
constexpr uint32_t VERDICT_NONE = 0xffu;  // finish has not judged the proof yet

// ---- out-of-line pieces of field.hpp / curve.hpp for these kernels (ZKR_HD is __forceinline__)
__device__ __noinline__ Fq fq_mul_c(const Fq &a, const Fq &b) { return mul(a, b); }
__device__ __noinline__ G1XYZZ g1_add_mixed_c(const G1XYZZ &acc, const G1Affine &q) { return add_mixed(acc, q); }
// 32 B little-endian standard form at p (4-byte aligned) -> words; false when the value is not below the modulus
template <class PM>
__device__ __forceinline__ bool load_below(const uint32_t *p, Fp<PM> &out) {
#pragma unroll
  for (int i = 0; i < 8; i++) out.v[i] = p[i];
  return words_below(out.v, PM::P);
}
__device__ __forceinline__ Fq fq_to_mont_c(const Fq &a) { return fq_mul_c(a, Fq::r2()); }

// public signal j of proof i: word 1 + j of its witness, or row i of the staged host signals
struct PublicSrc {
  const uint32_t *const *wit;  // null: the staged form
  const uint32_t *staged;
  uint32_t n_public;
  __device__ __forceinline__ const uint32_t *at(uint32_t i, uint32_t j) const {
    return wit ? wit[i] + 8 * (size_t)(1 + j) : staged + 8 * ((size_t)i * n_public + j);
  }
};

struct IngestArgs {
  const uint32_t *proofs;  // n x 64 words
  PublicSrc pub;
  const Consts *k;
  G1Affine *a, *c;         // a: -A
  G2Affine *b;
  uint32_t *verdict;
  uint32_t n;
};
__global__ void __launch_bounds__(VERIFY_THREADS) verify_ingest_kernel(IngestArgs g) {
  const uint32_t i = blockIdx.x * VERIFY_THREADS + threadIdx.x;
  if (i >= g.n) return;
  const uint32_t *pr = g.proofs + 64 * (size_t)i;
  const Consts &k = *g.k;
  Fq ax, ay, cx, cy;
  // A and C: coordinates below q, finite, on the curve
  if (!load_below(pr, ax) || !load_below(pr + 8, ay) || !load_below(pr + 48, cx) || !load_below(pr + 56, cy)) { g.verdict[i] = ZKR_VERDICT_BAD_G1; return; }
  G1Affine a{fq_to_mont_c(ax), fq_to_mont_c(ay)}, c{fq_to_mont_c(cx), fq_to_mont_c(cy)};
  if (a.is_inf() || c.is_inf() || !pairing::g1_on_curve(a, k) || !pairing::g1_on_curve(c, k)) { g.verdict[i] = ZKR_VERDICT_BAD_G1; return; }
  // every public signal below r, as it stands
  for (uint32_t j = 0; j < g.pub.n_public; j++) {
    Fr s;
    if (!load_below(g.pub.at(i, j), s)) { g.verdict[i] = ZKR_VERDICT_BAD_INPUT; return; }
  }
  // B: below q, finite, on the twist, in the order-r subgroup
  Fq bc[4];
  bool below = true;
  for (int t = 0; t < 4; t++) below = load_below(pr + 16 + 8 * t, bc[t]) && below;
  if (!below) { g.verdict[i] = ZKR_VERDICT_BAD_G2; return; }
  G2Affine b{Fq2{fq_to_mont_c(bc[0]), fq_to_mont_c(bc[1])}, Fq2{fq_to_mont_c(bc[2]), fq_to_mont_c(bc[3])}};
  if (b.is_inf() || !pairing::g2_on_curve(b, k) || !pairing::g2_in_subgroup(b, k)) { g.verdict[i] = ZKR_VERDICT_BAD_G2; return; }
  a.y = neg(a.y);
  g.a[i] = a;
  g.b[i] = b;
  g.c[i] = c;
  g.verdict[i] = VERDICT_NONE;
}

struct VkxArgs {
  PublicSrc pub;
  const G1Affine *win8;  // [j * 255 + d - 1] = d * IC_{j+1}
  G1Affine ic0;
  const uint32_t *verdict;
  G1Affine *vkx;
  uint32_t n;
};
__global__ void __launch_bounds__(VERIFY_THREADS) verify_vkx_kernel(VkxArgs g) {
  const uint32_t i = blockIdx.x * VERIFY_THREADS + threadIdx.x;
  if (i >= g.n || g.verdict[i] != VERDICT_NONE) return;
  G1XYZZ acc = G1XYZZ::inf();
  for (int w = 31; w >= 0; w--) {  // the windows of zkr_verify's ic_combination, most significant first
    if (w != 31)
      for (int t = 0; t < 8; t++) acc = dbl_xyzz(acc);
    for (uint32_t j = 0; j < g.pub.n_public; j++) {
      const uint32_t d = (g.pub.at(i, j)[w >> 2] >> (8 * (w & 3))) & 255u;
      if (d) acc = g1_add_mixed_c(acc, g.win8[(size_t)j * 255 + d - 1]);
    }
  }
  acc = add_full(acc, to_xyzz(g.ic0));
  g.vkx[i] = to_affine(acc);  // infinity: x = 0, and the pair contributes one
}

struct MillerArgs {
  const G1Affine *a, *c, *vkx;
  const G2Affine *b;
  const Line *gamma, *delta;
  const Consts *k;
  const uint32_t *verdict;
  uint32_t *degenerate;  // per proof: the projective loop of (-A, B) met Z = 0
  Fq12 *f;  // [pair][cap]
  uint32_t n, cap;
};
__global__ void __launch_bounds__(VERIFY_THREADS) verify_miller_kernel(MillerArgs g) {
  const uint32_t i = blockIdx.x * VERIFY_THREADS + threadIdx.x;
  if (i >= g.n || g.verdict[i] != VERDICT_NONE) return;  // the verdicts are only read here: finish judges
  const uint32_t pair = blockIdx.y;
  if (pair == 0) {
    bool ok;
    const G1Affine a = g.a[i];
    const G2Affine b = g.b[i];
    g.f[i] = pairing::miller_loop_proj(a, b, *g.k, &ok);
    g.degenerate[i] = ok ? 0u : 1u;
  } else {
    const G1Affine p = pair == 1 ? g.vkx[i] : g.c[i];
    g.f[(size_t)pair * g.cap + i] = pairing::miller_loop_prepared(p, pair == 1 ? g.gamma : g.delta);
  }
}

struct FinishArgs {
  const Fq12 *f, *f_alfa_beta;
  const Consts *k;
  const uint32_t *degenerate;
  uint32_t *verdict;
  uint32_t n, cap;
};
__global__ void __launch_bounds__(VERIFY_THREADS) verify_finish_kernel(FinishArgs g) {
  const uint32_t i = blockIdx.x * VERIFY_THREADS + threadIdx.x;
  if (i >= g.n || g.verdict[i] != VERDICT_NONE) return;
  // a degenerate step cannot happen for a B of order r, and is never "valid" (zkr_verify answers 0)
  if (g.degenerate[i]) { g.verdict[i] = ZKR_VERDICT_BAD_G2; return; }
  const Fq12 f_pub = g.f[(size_t)g.cap + i];
  const Fq12 f_proof = pairing::mul(g.f[i], g.f[2 * (size_t)g.cap + i]);
  const Fq12 f = pairing::mul(pairing::mul(*g.f_alfa_beta, f_pub), f_proof);
  g.verdict[i] = pairing::final_exponentiation(f, *g.k) == Fq12::one() ? ZKR_VERDICT_VALID : ZKR_VERDICT_EQUATION;
}

// the stage hook: e(P_i, Q_i), points as given
struct PairingArgs {
  const uint32_t *g1, *g2;  // n x 16, n x 32 words, standard form
  const Consts *k;
  uint32_t *out;            // n x 96 words
  uint8_t *degenerate;
  uint32_t n;
};
__global__ void __launch_bounds__(VERIFY_THREADS) pairing_kernel(PairingArgs g) {
  const uint32_t i = blockIdx.x * VERIFY_THREADS + threadIdx.x;
  if (i >= g.n) return;
  Fq c[6];
  for (int t = 0; t < 2; t++) { load_below(g.g1 + 16 * (size_t)i + 8 * t, c[t]); c[t] = fq_to_mont_c(c[t]); }
  for (int t = 0; t < 4; t++) { load_below(g.g2 + 32 * (size_t)i + 8 * t, c[2 + t]); c[2 + t] = fq_to_mont_c(c[2 + t]); }
  const G1Affine p{c[0], c[1]};
  const G2Affine q{Fq2{c[2], c[3]}, Fq2{c[4], c[5]}};
  bool ok;
  const Fq12 e = pairing::final_exponentiation(pairing::miller_loop_proj(p, q, *g.k, &ok), *g.k);
  const Fq2 *co[6] = {&e.c0.c0, &e.c0.c1, &e.c0.c2, &e.c1.c0, &e.c1.c1, &e.c1.c2};
  Fq one_std = Fq::zero();
  one_std.v[0] = 1;
  uint32_t *o = g.out + 96 * (size_t)i;
  for (int t = 0; t < 6; t++) {
    const Fq lo = fq_mul_c(co[t]->a, one_std), hi = fq_mul_c(co[t]->b, one_std);  // from_mont
    for (int w = 0; w < 8; w++) { o[16 * t + w] = lo.v[w]; o[16 * t + 8 + w] = hi.v[w]; }
  }
  g.degenerate[i] = ok ? 0 : 1;
}

}  // namespace zkr

namespace {
int upload(DevBuf &d, const void *src, size_t bytes) {
  if (int rc = d.alloc(bytes)) return rc;
  if (bytes) ZKR_HIP_CHECK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
void lines_of(const pairing::G2Prepared &p, std::vector<Line> &out) {
  for (size_t s = 0; s < p.lam.size(); s++) out.push_back(Line{p.lam[s], p.c[s]});
}
const char *verdict_text(unsigned v) {
  switch (v) {
    case ZKR_VERDICT_BAD_G1: return "A or C is not a finite point of the curve with coordinates below q";
    case ZKR_VERDICT_BAD_INPUT: return "a public signal is not below r";
    case ZKR_VERDICT_BAD_G2: return "B is not in the order-r subgroup";
    default: return "pairing equation fails";
  }
}
}  // namespace

struct zkr_vk {
  int device = 0;
  size_t n_public = 0;
  G1Affine ic0;
  DevBuf consts, win8, lines, f_alfa_beta;  // lines: beta | gamma | delta, N_LINES each
  OwnStream stream;
  ScopedEvent ev;
  // per-batch buffers, for `cap` proofs: they grow to the largest piece seen
  size_t cap = 0;
  DevBuf proofs, pub, wptrs, a, b, c, vkx, f, verdict, degenerate;
  Pinned<uint32_t> h_verdict;
};

namespace {
int vk_reserve(zkr_vk *vk, size_t n) {
  if (n <= vk->cap) return 0;
  for (DevBuf *d : {&vk->proofs, &vk->pub, &vk->wptrs, &vk->a, &vk->b, &vk->c, &vk->vkx, &vk->f, &vk->verdict, &vk->degenerate})
    d->reset();  // all of the old ones before any of the new
  vk->h_verdict.reset();
  vk->cap = 0;
  int rc;
  if ((rc = vk->proofs.alloc(n * 256)) || (rc = vk->pub.alloc(n * vk->n_public * 32)) || (rc = vk->wptrs.alloc(n * sizeof(void *))) ||
      (rc = vk->a.alloc(n * sizeof(G1Affine))) || (rc = vk->b.alloc(n * sizeof(G2Affine))) || (rc = vk->c.alloc(n * sizeof(G1Affine))) ||
      (rc = vk->vkx.alloc(n * sizeof(G1Affine))) || (rc = vk->f.alloc(3 * n * sizeof(Fq12))) || (rc = vk->verdict.alloc(n * 4)) || (rc = vk->degenerate.alloc(n * 4)))
    return rc;
  if ((rc = vk->h_verdict.alloc(n))) return rc;
  vk->cap = n;
  return 0;
}

// one piece (nb <= ZKR_VERIFY_PIECE proofs) on the handle's stream; its verdicts in vk->h_verdict when this returns
int verify_piece(zkr_vk *vk, const uint8_t *proofs, const void *publics_std, const void *const *d_wit, size_t nb) {
  if (int rc = vk_reserve(vk, nb)) return rc;
  const hipStream_t st = vk->stream;
  ZKR_HIP_CHECK(hipMemcpyAsync(vk->proofs.p, proofs, nb * 256, hipMemcpyHostToDevice, st));
  if (d_wit) ZKR_HIP_CHECK(hipMemcpyAsync(vk->wptrs.p, d_wit, nb * sizeof(void *), hipMemcpyHostToDevice, st));
  else if (vk->n_public) ZKR_HIP_CHECK(hipMemcpyAsync(vk->pub.p, publics_std, nb * vk->n_public * 32, hipMemcpyHostToDevice, st));
  const PublicSrc pub{d_wit ? vk->wptrs.as<const uint32_t *const>() : nullptr, vk->pub.as<uint32_t>(), (uint32_t)vk->n_public};
  const Consts *k = vk->consts.as<Consts>();
  const unsigned blocks = (unsigned)((nb + VERIFY_THREADS - 1) / VERIFY_THREADS);
  const uint32_t n = (uint32_t)nb, cap = (uint32_t)vk->cap;
  verify_ingest_kernel<<<blocks, VERIFY_THREADS, 0, st>>>(IngestArgs{vk->proofs.as<uint32_t>(), pub, k, vk->a.as<G1Affine>(), vk->c.as<G1Affine>(), vk->b.as<G2Affine>(), vk->verdict.as<uint32_t>(), n});
  verify_vkx_kernel<<<blocks, VERIFY_THREADS, 0, st>>>(VkxArgs{pub, vk->win8.as<G1Affine>(), vk->ic0, vk->verdict.as<uint32_t>(), vk->vkx.as<G1Affine>(), n});
  const Line *lines = vk->lines.as<Line>();
  verify_miller_kernel<<<dim3(blocks, 3), VERIFY_THREADS, 0, st>>>(MillerArgs{vk->a.as<G1Affine>(), vk->c.as<G1Affine>(), vk->vkx.as<G1Affine>(), vk->b.as<G2Affine>(), lines + pairing::N_LINES, lines + 2 * pairing::N_LINES, k, vk->verdict.as<uint32_t>(), vk->degenerate.as<uint32_t>(), vk->f.as<Fq12>(), n, cap});
  verify_finish_kernel<<<blocks, VERIFY_THREADS, 0, st>>>(FinishArgs{vk->f.as<Fq12>(), vk->f_alfa_beta.as<Fq12>(), k, vk->degenerate.as<uint32_t>(), vk->verdict.as<uint32_t>(), n, cap});
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpyAsync(vk->h_verdict, vk->verdict.p, nb * 4, hipMemcpyDeviceToHost, st));
  ZKR_HIP_CHECK(hipStreamSynchronize(st));
  return 0;
}

int verify_each(zkr_vk *vk, const uint8_t *proofs, const void *publics_std, const void *const *d_wit, size_t n_proofs, void *stream, uint8_t *verdicts, int *all_valid) {
  *all_valid = 0;
  if (n_proofs == 0) { *all_valid = 1; return 0; }
  ZKR_HIP_CHECK(hipSetDevice(vk->device));
  if (d_wit) {  // the witnesses are in place once the caller's stream has come this far
    ZKR_HIP_CHECK(hipEventRecord(vk->ev, (hipStream_t)stream));
    ZKR_HIP_CHECK(hipStreamWaitEvent(vk->stream, vk->ev, 0));
  }
  size_t first_bad = n_proofs;
  unsigned first_code = 0;
  for (size_t j0 = 0; j0 < n_proofs; j0 += ZKR_VERIFY_PIECE) {
    const size_t nb = n_proofs - j0 < ZKR_VERIFY_PIECE ? n_proofs - j0 : ZKR_VERIFY_PIECE;
    const uint8_t *pub = publics_std ? (const uint8_t *)publics_std + j0 * vk->n_public * 32 : nullptr;
    if (int rc = verify_piece(vk, proofs + 256 * j0, pub, d_wit ? d_wit + j0 : nullptr, nb)) return rc;
    for (size_t j = 0; j < nb; j++) {
      const unsigned v = vk->h_verdict[j];
      if (v > ZKR_VERDICT_EQUATION) { set_error("proof %zu: the device left no verdict (%u)", j0 + j, v); return ZKR_ERR_HIP; }
      if (verdicts) verdicts[j0 + j] = (uint8_t)v;
      if (v && first_bad == n_proofs) { first_bad = j0 + j; first_code = v; }
    }
  }
  *all_valid = first_bad == n_proofs ? 1 : 0;
  if (first_bad != n_proofs) set_error("proof %zu: %s", first_bad, verdict_text(first_code));
  return 0;
}
}  // namespace

extern "C" {

int zkr_vk_load(const void *vk_bin, size_t vk_len, int device, zkr_vk **out) {
  if (!vk_bin || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  *out = nullptr;
  // nPublic from the key's own IC count; everything else is parse_vk's business, before any device call
  size_t n_public = 0;
  if (vk_len >= VK_FIXED_BYTES) {
    const uint32_t n_ic = vk_ic_count(vk_bin);
    if (n_ic) n_public = n_ic - 1;
  }
  ParsedVk pk;
  if (int rc = parse_vk(vk_bin, vk_len, n_public, pk)) return rc;
  pairing::G2Prepared prep[3];
  if (!pairing::g2_prepare(pk.beta2, prep[0]) || !pairing::g2_prepare(pk.gamma2, prep[1]) || !pairing::g2_prepare(pk.delta2, prep[2])) {
    set_error("verifying key: a G2 point is not a valid pairing input");
    return ZKR_ERR_BAD_KEY;
  }
  if (int rc = need_device(device)) return rc;
  std::vector<Line> lines;
  for (int t = 0; t < 3; t++) {
    if (prep[t].lam.size() != (size_t)pairing::N_LINES) { set_error("verifying key: %zu prepared lines, expected %d", prep[t].lam.size(), pairing::N_LINES); return ZKR_ERR_BAD_KEY; }
    lines_of(prep[t], lines);
  }
  const pairing::G2Prepared *qb = &prep[0];
  const Fq12 fab = pairing::miller_loop_mixed(nullptr, nullptr, 0, &pk.alfa1, &qb, 1);  // both arguments belong to the key, as in the host cache
  std::vector<G1Affine> win8;
  build_win8(pk.ics, win8);
  const Consts k = pairing::host_consts();
  zkr_vk *vk = new zkr_vk();
  vk->device = device;
  vk->n_public = n_public;
  vk->ic0 = pk.ic0;
  int rc = 0;
  auto setup = [&]() -> int {
    ZKR_HIP_CHECK(hipSetDevice(device));
    if ((rc = upload(vk->consts, &k, sizeof(k))) || (rc = upload(vk->win8, win8.data(), win8.size() * sizeof(G1Affine))) ||
        (rc = upload(vk->lines, lines.data(), lines.size() * sizeof(Line))) || (rc = upload(vk->f_alfa_beta, &fab, sizeof(fab))))
      return rc;
    if (int src = vk->stream.create()) return src;
    if (int erc = vk->ev.create(hipEventDisableTiming)) return erc;
    return 0;
  };
  if ((rc = setup())) { delete vk; return rc; }
  *out = vk;
  return 0;
}

void zkr_vk_free(zkr_vk *vk) {
  if (!vk) return;
  (void)hipSetDevice(vk->device);
  delete vk;
}

int zkr_vk_info(const zkr_vk *vk, uint64_t out[2]) {
  if (!vk || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  out[0] = vk->n_public;
  out[1] = (uint64_t)vk->device;
  return 0;
}

int zkr_verify_each(zkr_vk *vk, const uint8_t *proofs, const void *publics_std, size_t n_proofs, uint8_t *verdicts, int *all_valid) {
  if (!vk || !all_valid || (n_proofs && (!proofs || (vk->n_public && !publics_std)))) { set_error("null argument"); return ZKR_ERR_ARG; }
  return verify_each(vk, proofs, publics_std, nullptr, n_proofs, nullptr, verdicts, all_valid);
}

int zkr_verify_each_device(zkr_vk *vk, const uint8_t *proofs, const void *const *d_witnesses_std, size_t n_proofs, void *stream, uint8_t *verdicts, int *all_valid) {
  if (!vk || !all_valid || (n_proofs && (!proofs || !d_witnesses_std))) { set_error("null argument"); return ZKR_ERR_ARG; }
  for (size_t j = 0; j < n_proofs; j++)
    if (!d_witnesses_std[j]) { set_error("witness %zu is a null pointer", j); return ZKR_ERR_ARG; }
  return verify_each(vk, proofs, nullptr, d_witnesses_std, n_proofs, stream, verdicts, all_valid);
}

int zkr_pairing_device(const void *g1_std, const void *g2_std, size_t n, void *out, uint8_t *degenerate, int device) {
  if (n && (!g1_std || !g2_std || !out)) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (n > 0xffffffffull / 96) { set_error("%zu pairs are more than one call takes", n); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  if (n == 0) return 0;
  ZKR_HIP_CHECK(hipSetDevice(device));
  const Consts k = pairing::host_consts();
  DevBuf dk, d1, d2, dout, ddeg;
  int rc;
  if ((rc = upload(dk, &k, sizeof(k))) || (rc = upload(d1, g1_std, n * 64)) || (rc = upload(d2, g2_std, n * 128)) || (rc = dout.alloc(n * 384)) || (rc = ddeg.alloc(n))) return rc;
  pairing_kernel<<<(unsigned)((n + VERIFY_THREADS - 1) / VERIFY_THREADS), VERIFY_THREADS>>>(PairingArgs{d1.as<uint32_t>(), d2.as<uint32_t>(), dk.as<Consts>(), dout.as<uint32_t>(), ddeg.as<uint8_t>(), (uint32_t)n});
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpy(out, dout.p, n * 384, hipMemcpyDeviceToHost));
  if (degenerate) ZKR_HIP_CHECK(hipMemcpy(degenerate, ddeg.p, n, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
