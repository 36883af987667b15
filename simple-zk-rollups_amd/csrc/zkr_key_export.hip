// zkr_key_export.hip -- a device key back in the byte layout it may have come from: the provingKeyBin that binarifyProvingKey
// writes (the reference's operator/src/utils/binarify.ts:143-206) and groth16GenProof reads (operator/src/snarks/common.ts:28-29).
// The way in is zkr_key_load_websnark (zkr_key.hip); this is its inverse for ANY whole key, whoever built the arena -- a setup from
// a transcript and the contributions after it have no other way to the reference's own prover.
//
// What comes from where: n, p, m and the 448 constant bytes from the arena header; polsA / polsB from the two CSR sides, which go
// to the host as the three arrays they are and are transposed there (websnark_writer.cpp); the five point sections from level 0 of
// the window tables through the rank maps, on the device, a piece of the output at a time.
#include <chrono>
#include "curve29.hpp"
#include "websnark_writer.hpp"
#include "zkr_internal.hpp"

namespace zkr {

// the scalar a slot of an output section belongs to: slot + shift (A, B1, B2: 0; C: nPublic + 1), or for hExps the bit reversal
// of the slot over rev_bits = log2 m bits -- the loader pairs scalar position j with hExps[bitrev(j)] (zkr_key_load_websnark)
struct SlotMap {
  uint32_t shift, rev_bits;
};

// packed canonical x 2^261 -> packed canonical standard form: the Montgomery product with the INTEGER one takes the radix off.
// On coordinates in memory and with the inline canonical_small, as radix_to_256_at (curve29.hpp) and for its reason: no stack frame.
template <class F>
ZKR_HD_COLD void radix_to_std_at(F *w);
template <>
ZKR_HD_COLD void radix_to_std_at<Fq>(Fq *w) {
  L29<Fq29, 2> one = L29<Fq29, 2>::zero();
  one.v[0] = 1;
  *w = G1C::pack<2>(canonical_small(mul(G1C::unpack<10>(*w), one)));
}
template <>
ZKR_HD_COLD void radix_to_std_at<Fq2>(Fq2 *w) {
  L29<Fq29, 2> one = L29<Fq29, 2>::zero();
  one.v[0] = 1;
  *w = G2C::pack<2>(canonical_small(mul(G2C::unpack<10>(*w), Q29<2>{one, L29<Fq29, 2>::zero()})));
}

// out[i] = the wire form of the point that multiplies the scalar of slot lo + i, one thread per output point.  lvl0: level 0 of
// the table (npts points, x 2^261 canonical; x = 0: the placeholder of a table laid out over a shared support); rank: the table's
// rank map, null when the header says it is the identity.  No point (RANK_NONE, a placeholder) is the point at infinity as
// binarify.ts:92-102 writes snarkjs's [0, 1, 0]: x = 0, y = one -- Montgomery one, or the integer with `standard`.  The point moves
// in 16-byte pieces, as in gather_kernel, and is converted where it lands: no lane holds a whole point.
template <class F>
static __global__ __launch_bounds__(256) void export_points_kernel(const Affine<F> *lvl0, uint32_t npts, const uint32_t *rank, SlotMap mp, uint32_t lo, uint32_t count,
                                                                   int standard, Affine<F> *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t slot = lo + i;
  const uint32_t s = mp.rev_bits ? __brev(slot) >> (32 - mp.rev_bits) : slot + mp.shift;
  const uint32_t r = rank ? rank[s] : s;
  constexpr unsigned HALF = sizeof(F) / 16;  // pieces per coordinate
  uint4 *o = reinterpret_cast<uint4 *>(out + i);
  uint32_t any = 0;
  if (r < npts) {  // RANK_NONE is above every count
    const uint4 *src = reinterpret_cast<const uint4 *>(lvl0 + r);
#pragma unroll
    for (unsigned k = 0; k < HALF; k++) {
      const uint4 v = src[k];
      any |= v.x | v.y | v.z | v.w;
      o[k] = v;
    }
    if (any) {
#pragma unroll
      for (unsigned k = HALF; k < 2 * HALF; k++) o[k] = src[k];
    }
  }
  if (!any) {
    const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (unsigned k = 0; k < 2 * HALF; k++) o[k] = zero;
    o[HALF] = standard ? make_uint4(1, 0, 0, 0) : make_uint4(FqParams::R1[0], FqParams::R1[1], FqParams::R1[2], FqParams::R1[3]);
    if (!standard) o[HALF + 1] = make_uint4(FqParams::R1[4], FqParams::R1[5], FqParams::R1[6], FqParams::R1[7]);
    return;
  }
  if (standard) { radix_to_std_at(&out[i].x); radix_to_std_at(&out[i].y); } else { radix_to_256_at(&out[i].x); radix_to_256_at(&out[i].y); }
}

namespace {
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
// the last export of this thread: kernels, copies, host writer, total (ms), extra device bytes at the peak
thread_local double g_last[5] = {0, 0, 0, 0, 0};

// what one export owns: a staging buffer of `piece` G2 points on the device, a pinned buffer at least as large, one stream
struct ExportScratch {
  DevBuf stage;
  PinnedBuf pinned;
  OwnStream stream;
  size_t pinned_bytes = 0;
  double ms_copy = 0, ms_kernel = 0;
  // `bytes` of device memory to the host through the pinned buffer, on the call's own stream
  int download(void *dst, const void *d_src, size_t bytes) {
    const auto t0 = Clock::now();
    for (size_t off = 0; off < bytes; off += pinned_bytes) {
      const size_t nb = bytes - off < pinned_bytes ? bytes - off : pinned_bytes;
      ZKR_HIP_CHECK(hipMemcpyAsync(pinned, (const uint8_t *)d_src + off, nb, hipMemcpyDeviceToHost, stream));
      ZKR_HIP_CHECK(hipStreamSynchronize(stream));
      memcpy((uint8_t *)dst + off, pinned, nb);
    }
    ms_copy += ms_since(t0);
    return 0;
  }
};

struct FreeHost { void operator()(void *p) const { free(p); } };
}  // namespace

static int key_export(const zkr_key *k, uint32_t flags, uint32_t piece_points, void **pk_out, size_t *pk_len) {
  const ArenaHeader &h = k->h;
  const bool standard = (flags & ZKR_EXPORT_STANDARD) != 0;
  const auto t_all = Clock::now();
  WebsnarkPlan pl;
  if (int rc = websnark_plan(h.n, h.p, h.m, h.nnzA, h.nnzB, pl)) return rc;  // before anything is allocated
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  uint64_t piece = piece_points ? piece_points : (1u << 20);
  uint64_t most = 1;
  for (int t = 0; t < N_TABLES; t++) most = pl.count[t] > most ? pl.count[t] : most;
  if (piece > most) piece = most;
  ExportScratch sc;
  sc.pinned_bytes = (size_t)piece * 128 > ((size_t)1 << 16) ? (size_t)piece * 128 : ((size_t)1 << 16);
  int rc;
  if ((rc = sc.stage.alloc((size_t)piece * 128)) || (rc = sc.pinned.alloc(sc.pinned_bytes)) || (rc = sc.stream.create())) return rc;
  Owner<void *, FreeHost> out;
  out.p = malloc(pl.len);
  if (!out.p) { set_error("no host memory for %llu bytes", (unsigned long long)pl.len); return ZKR_ERR_ARG; }
  uint8_t *o = (uint8_t *)out.p;

  // the two QAP sides, then header and pols sections on the host
  double ms_host = 0;
  {
    std::vector<uint32_t> rowptr[2], col[2];
    std::vector<uint8_t> coef[2];
    for (int s = 0; s < 2; s++) {
      const size_t nnz = s == 0 ? h.nnzA : h.nnzB;
      rowptr[s].resize((size_t)h.m + 1);
      col[s].resize(nnz + 1);
      coef[s].resize(nnz * 32 + 32);
      if ((rc = sc.download(rowptr[s].data(), k->arena + h.off_rowptr[s], ((size_t)h.m + 1) * 4)) || (rc = sc.download(col[s].data(), k->arena + h.off_col[s], nnz * 4)) ||
          (rc = sc.download(coef[s].data(), k->arena + h.off_coef[s], nnz * 32)))
        return rc;
    }
    const auto t0 = Clock::now();
    uint8_t consts[448];
    header_get_consts(h, consts);
    if (standard) {  // x 2^-256: the 14 coordinates of the header, every coefficient
      for (int c = 0; c < 14; c++) {
        Fq v;
        memcpy(v.v, consts + 32 * c, 32);
        v = from_mont(v);
        memcpy(consts + 32 * c, v.v, 32);
      }
      for (int s = 0; s < 2; s++) {
        const size_t nnz = s == 0 ? h.nnzA : h.nnzB;
        for (size_t e = 0; e < nnz; e++) {
          Fr v;
          memcpy(v.v, &coef[s][e * 32], 32);
          v = from_mont(v);
          memcpy(&coef[s][e * 32], v.v, 32);
        }
      }
    }
    const uint32_t *rp[2] = {rowptr[0].data(), rowptr[1].data()}, *cl[2] = {col[0].data(), col[1].data()};
    const uint8_t *cf[2] = {coef[0].data(), coef[1].data()};
    if ((rc = websnark_write_front(o, pl, h.n, h.p, h.m, consts, rp, cl, cf))) return rc;
    ms_host += ms_since(t0);
  }

  // the five point sections, a piece at a time: kernel into the staging buffer, copy to the pinned buffer, from there to its place
  for (int t = 0; t < N_TABLES; t++) {
    const size_t pb = WEBSNARK_POINT_BYTES[t];
    const SlotMap mp{t == T_C ? h.p + 1 : 0u, t == T_H ? h.logm : 0u};
    const uint32_t *rank = h.rank_identity[t] ? nullptr : (const uint32_t *)(k->arena + h.off_rank[t]);
    for (uint64_t lo = 0; lo < pl.count[t]; lo += piece) {
      const uint32_t cnt = (uint32_t)(pl.count[t] - lo < piece ? pl.count[t] - lo : piece);
      const unsigned grid = (cnt + 255) / 256;
      const auto t0 = Clock::now();
      if (t == T_B2)
        export_points_kernel<Fq2><<<grid, 256, 0, sc.stream>>>((const G2Affine *)(k->arena + h.off_pts[t]), h.npts[t], rank, mp, (uint32_t)lo, cnt, standard ? 1 : 0, sc.stage.as<G2Affine>());
      else
        export_points_kernel<Fq><<<grid, 256, 0, sc.stream>>>((const G1Affine *)(k->arena + h.off_pts[t]), h.npts[t], rank, mp, (uint32_t)lo, cnt, standard ? 1 : 0, sc.stage.as<G1Affine>());
      ZKR_HIP_CHECK(hipGetLastError());
      ZKR_HIP_CHECK(hipStreamSynchronize(sc.stream));
      sc.ms_kernel += ms_since(t0);
      if ((rc = sc.download(o + pl.ptr[2 + t] + lo * pb, sc.stage, (size_t)cnt * pb))) return rc;
    }
  }
  g_last[0] = sc.ms_kernel; g_last[1] = sc.ms_copy; g_last[2] = ms_host; g_last[3] = ms_since(t_all);
  g_last[4] = (double)((size_t)piece * 128);
  *pk_out = out.release();
  *pk_len = pl.len;
  return 0;
}

}  // namespace zkr

using namespace zkr;

extern "C" int zkr_key_export_websnark(const zkr_key *key, const zkr_key_export_opts *opts, void **pk_out, size_t *pk_len) {
  const uint32_t flags = opts ? opts->flags : 0;
  if (flags & ~ZKR_EXPORT_STANDARD) { set_error("unknown export flag 0x%x", flags & ~ZKR_EXPORT_STANDARD); return ZKR_ERR_ARG; }
  if (!key || !pk_out || !pk_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (key->h.shard_parts != 1) { set_error("a shard holds a range of the tables: export the whole key it was cut from"); return ZKR_ERR_ARG; }
  if (int rc = need_device(key->device, "zkr_key_export_websnark")) return rc;
  return key_export(key, flags, opts ? opts->piece_points : 0, pk_out, pk_len);
}

extern "C" int zkr_key_export_last_times(double out[5]) {
  if (!out) { set_error("null argument"); return ZKR_ERR_ARG; }
  for (int i = 0; i < 5; i++) out[i] = g_last[i];
  return 0;
}
