// kernels_group.hpp -- arithmetic on VECTORS OF GROUP ELEMENTS, which the proving path never needs (its points are fixed, its
// scalars vary) and a powers-of-tau transcript is made of: every point multiplied by a scalar of its own, and the radix-2 NTT
// whose coefficients are points (the Lagrange-basis form of tau^i G).  The delta contribution's kernel (every point times ONE
// scalar, zkr_contribute.hip), the curve-equation check of the key loader and the slot-by-slot addition of the side tables a key
// derives from its own points (zkr_eval_tables.hip) are here too: one home for them all.  Templated over the coordinate families of curve29.hpp
// (G1C over Fq, G2C over Fq2); the group law is the hot path's (XYZZ accumulator, dbl_xyzz29, add_mixed29).
//
// Points are affine in the key's boundary radix (x 2^256; x == 0 = infinity) in memory, in and out, as zkr_msm_g1 / g2 take them.
// A kernel leaves its results unnormalised -- X, Y in the point's own slot, ZZ, ZZZ in `ztmp` ([2][n] coordinates) -- and each
// thread makes its own results affine with ONE inversion of the product of their ZZZ (x = X ZZ^2 / ZZZ^2, y = Y / ZZZ, since
// ZZ^3 = ZZZ^2), as msm_precompute_kernel does over its levels.
//
// Per-lane scalars: the 64 lanes of a wavefront hold 64 different scalars, so "add where the bit is set" runs for the wave in
// practically every step whatever form the digits take (a signed form saves nothing: some lane always has a non-zero digit).  The
// ladder is therefore the plain one -- 254 doublings, the addition under the lane's bit, which the execution mask turns into
// "compute for all, keep where set" -- and it reads the scalar's bits from memory (one cached word per 32 steps' worth): no
// per-thread digit array and no table of multiples, either of which would be indexed at run time and live in scratch.
// Fq products: 254 x (9 + 11) = 5.1e3 per G1 multiplication; an Fq2 product is three to four of them.
#pragma once
#include "kernels_msm.hpp"  // load_pod / store_pod, curve29.hpp
#include "kernels_ntt.hpp"  // load_fr / store_fr, twiddle_table_kernel
#include "pairing.hpp"      // the curve constants

namespace zkr {

constexpr int GROUP_THREADS = 256;
constexpr int GROUP_MAX_PTS = 8;   // points one thread of a scaling kernel multiplies and normalises together
constexpr int GROUP_SCALAR_BITS = 254;  // scalars are below r < 2^254
// Blocks of a scaling launch over n points, and the points a thread takes: one while that leaves the chip short of wavefronts
// (4 per SIMD on 1024 SIMDs), up to GROUP_MAX_PTS.
inline unsigned group_scale_grid(size_t n, int *npt) {
  const size_t per = n / (1024u * 64u * 4u);
  *npt = per < 1 ? 1 : per > (size_t)GROUP_MAX_PTS ? GROUP_MAX_PTS : (int)per;
  const size_t threads = (n + (size_t)*npt - 1) / (size_t)*npt;
  return (unsigned)((threads + GROUP_THREADS - 1) / GROUP_THREADS);
}

// a checking kernel's tally: bad[0] = entries that fail, bad[1] = the smallest index among them (host side: FaultCounter)
__device__ __forceinline__ void group_note_bad(uint32_t *bad, uint32_t i) {
  atomicAdd(&bad[0], 1u);
  atomicMin(&bad[1], i);
}

// packed affine x 2^256 -> registers x 2^261 (canonical); the caller has filtered infinity
template <class C>
__device__ __forceinline__ Affine29<C> group_affine_in(const Affine<typename C::W> &p) {
  return Affine29<C>{canonical_small(mul(C::template unpack<10>(p.x), C::to261())), canonical_small(mul(C::template unpack<10>(p.y), C::to261()))};
}

// k q, k = 8 words in memory, standard form below 2^bits
template <class C>
__device__ __forceinline__ XYZZ29<C> group_lane_mul(const Affine29<C> &q, const uint32_t *k, int bits = GROUP_SCALAR_BITS) {
  XYZZ29<C> acc = XYZZ29<C>::inf();
#pragma unroll 1
  for (int b = bits - 1; b >= 0; b--) {
    acc = dbl_xyzz29<C>(acc);
    if ((k[b >> 5] >> (b & 31)) & 1u) acc = add_mixed29<C>(acc, q, false);
  }
  return acc;
}

// e q for ONE e common to all lanes, in signed-binary (NAF) form: `naf` = 16 words in device memory, [0..7] bit b set = digit b is
// non-zero, [8..15] bit b set = it is -1; `top` = index of the leading digit (always +1).  The digits are wave-uniform: read
// through the scalar unit and branched on uniformly, the -1 digits by add_mixed29's neg_q flag.
template <class C>
__device__ __forceinline__ XYZZ29<C> group_uniform_mul(const Affine29<C> &q, const uint32_t *naf, int top) {
  XYZZ29<C> acc = make_xyzz<C>(q.x, q.y, C::one(), C::one());  // the leading digit
#pragma unroll 1
  for (int b = top - 1; b >= 0; b--) {
    acc = dbl_xyzz29<C>(acc);
    const uint32_t nz = __builtin_amdgcn_readfirstlane(naf[b >> 5]), sg = __builtin_amdgcn_readfirstlane(naf[8 + (b >> 5)]);
    if ((nz >> (b & 31)) & 1u) acc = add_mixed29<C>(acc, q, ((sg >> (b & 31)) & 1u) != 0);
  }
  return acc;
}

// -p
template <class C>
__device__ __forceinline__ XYZZ29<C> group_neg(const XYZZ29<C> &p) {
  if (p.is_inf()) return p;
  XYZZ29<C> r = p;
  r.y = neg(p.y).template to<HY>();
  return r;
}

// result i of this thread, unnormalised; `prod` collects the ZZZ of the thread's finite results
template <class C, class P>
__device__ __forceinline__ void group_store_unnormalised(Affine<typename C::W> *pts, typename C::W *ztmp, size_t n, size_t i, const XYZZ29<C> &acc, P &prod) {
  using W = typename C::W;
  if (acc.is_inf()) {  // stored as infinity, a factor of one
    store_pod(pts + i, Affine<W>{W::zero(), W::zero()});
    store_pod(ztmp + i, W::zero());
    store_pod(ztmp + n + i, C::template pack<2>(C::one()));
    return;
  }
  store_pod(pts + i, Affine<W>{C::template pack<3>(weak(acc.x)), C::template pack<HY>(acc.y)});
  store_pod(ztmp + i, C::template pack<HY>(acc.zz));
  store_pod(ztmp + n + i, C::template pack<HY>(acc.zzz));
  prod = mul(prod, acc.zzz).template to<4>();
}

// the thread's results base + j step, j < cnt, made affine (x 2^256, canonical) with one inversion of `prod`
template <class C, class P>
__device__ __forceinline__ void group_normalise_own(Affine<typename C::W> *pts, typename C::W *ztmp, size_t n, size_t base, size_t step, int cnt, const P &prod) {
  using W = typename C::W;
  auto inv = inv29(prod);  // 1 / (ZZZ_0 ... ZZZ_{cnt-1})
#pragma unroll 1
  for (int j = cnt - 1; j >= 0; j--) {
    const size_t i = base + (size_t)j * step;
    auto pre = C::one().template to<4>();  // ZZZ_0 ... ZZZ_{j-1}
#pragma unroll 1
    for (int l = 0; l < j; l++) pre = mul(pre, C::template unpack<HY>(load_pod(ztmp + n + base + (size_t)l * step))).template to<4>();
    const auto zzz = C::template unpack<HY>(load_pod(ztmp + n + i));
    const auto izzz = mul(inv, pre);  // 1 / ZZZ_j
    inv = mul(inv, zzz).template to<4>();
    const auto zz = C::template unpack<HY>(load_pod(ztmp + i));
    if (zz.all_zero()) continue;  // infinity
    const auto izz = mul(sqr(zz), sqr(izzz));
    const Affine<W> a = load_pod(pts + i);
    const auto x = mul(C::template unpack<3>(a.x), izz), y = mul(C::template unpack<HY>(a.y), izzz);
    store_pod(pts + i, Affine<W>{C::template pack<2>(canonical_small(mul(x, C::to256()))), C::template pack<2>(canonical_small(mul(y, C::to256())))});
  }
}

// The frame of the two scaling kernels: pts[i] <- mul(q_i, i) in place, infinity staying infinity.  A thread takes up to `npt`
// points at stride = the launch's threads, so a wavefront's loads stay contiguous, and normalises them with one inversion.
// Its count is worked out BEFORE the loop: updated inside it, the uniform kernel needs 169-170 VGPRs, and 168 is the last
// allocation that lets three wavefronts share a SIMD.
// The store writes zeros over an infinity slot; the placeholders of a shared-support table (key_build) are all-zero already,
// so a key's bytes come out as if the slot had been left alone.
template <class C, class Mul>
__device__ __forceinline__ void group_scale_frame(Affine<typename C::W> *pts, uint32_t n, int npt, typename C::W *ztmp, Mul mul_point) {
  const uint32_t stride = gridDim.x * GROUP_THREADS, t0 = blockIdx.x * GROUP_THREADS + threadIdx.x;
  const int cnt = t0 < n ? (int)min((uint32_t)npt, (n - 1 - t0) / stride + 1) : 0;
  auto prod = C::one().template to<4>();
#pragma unroll 1
  for (int j = 0; j < cnt; j++) {
    const uint32_t i = t0 + (uint32_t)j * stride;
    const Affine<typename C::W> p = load_pod(pts + i);
    XYZZ29<C> acc = XYZZ29<C>::inf();
    if (!p.is_inf()) acc = mul_point(group_affine_in<C>(p), i);
    group_store_unnormalised<C>(pts, ztmp, n, i, acc, prod);
  }
  group_normalise_own<C>(pts, ztmp, n, t0, stride, cnt, prod);
}

// pts[i] <- s[i] pts[i].  scalars: 8 words each, standard form below r; scalar i is at scalars + 8 i sc_stride (sc_stride = 0:
// one scalar for all points, every branch of the ladder then uniform across the wavefront).
template <class C>
static __global__ __launch_bounds__(GROUP_THREADS) void group_scale_each_kernel(Affine<typename C::W> *pts, uint32_t n, int npt, const uint32_t *scalars, uint32_t sc_stride,
                                                                                 typename C::W *ztmp) {
  group_scale_frame<C>(pts, n, npt, ztmp, [=](const Affine29<C> &q, uint32_t i) { return group_lane_mul<C>(q, scalars + 8 * (uint64_t)i * sc_stride); });
}

// pts[i] <- e pts[i] for ONE scalar e in the form group_uniform_mul reads: no per-lane digit storage and no table of multiples.
// A delta contribution's C and H tables; `naf` is then the only device copy of the secret scalar, and the caller wipes it.
// Fq products, for the accounting beside the measured times (tools/contribution_time.py): dbl_xyzz29 = 9 (4
// squares + 3 products + the two-product Y form), add_mixed29 = 11 (2 squares + 7 products + the two-product Y form).  Per
// point: `top` doublings, one addition per non-zero digit below the leading one, 2 products for the radix change in, ~9 + npt / 2
// for the way back out, and 1 / npt of an inversion (253 squares + one product per set bit of p - 2).
template <class C>
static __global__ __launch_bounds__(GROUP_THREADS) void group_scale_uniform_kernel(Affine<typename C::W> *pts, uint32_t n, int npt, const uint32_t *naf, int top, typename C::W *ztmp) {
  group_scale_frame<C>(pts, n, npt, ztmp, [=](const Affine29<C> &q, uint32_t) { return group_uniform_mul<C>(q, naf, top); });
}

// One radix-2 stage of the NTT over points, decimation in time on bit-reversed input, in place: thread t owns the butterfly
// (u, v) = (pts[i], pts[i + half]) -> (u + w v, u - w v), i = 2 half (t / half) + j, j = t mod half, w = tw[j tw_stride]
// (tw: powers of the n-th root, 8 words each, STANDARD form; tw_stride = n / (2 half)).  w v by the ladder above; j = 0 (w = 1, every
// butterfly of the first stage) skips it.  Both outputs come from the XYZZ value T = w v and the affine u by the mixed addition:
// u + T, and u - T = -(T - u).  The two results share one inversion.
template <class C>
static __global__ __launch_bounds__(GROUP_THREADS) void group_butterfly_kernel(Affine<typename C::W> *pts, uint32_t n, uint32_t half, const uint32_t *tw, uint32_t tw_stride,
                                                                                typename C::W *ztmp) {
  const uint32_t t = blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (t >= n / 2) return;
  const uint32_t j = t & (half - 1);
  const size_t i = ((size_t)(t - j) << 1) | j;
  const Affine<typename C::W> v = load_pod(pts + i + half);
  XYZZ29<C> T = XYZZ29<C>::inf();
  if (!v.is_inf()) {
    const Affine29<C> q = group_affine_in<C>(v);
    if (j == 0) T = make_xyzz<C>(q.x, q.y, C::one(), C::one());
    else T = group_lane_mul<C>(q, tw + 8 * (size_t)j * tw_stride);
  }
  const Affine<typename C::W> u = load_pod(pts + i);
  auto prod = C::one().template to<4>();
  if (u.is_inf()) {
    group_store_unnormalised<C>(pts, ztmp, n, i, T, prod);
    group_store_unnormalised<C>(pts, ztmp, n, i + half, group_neg<C>(T), prod);
  } else {
    const Affine29<C> q = group_affine_in<C>(u);
    group_store_unnormalised<C>(pts, ztmp, n, i, add_mixed29<C>(T, q, false), prod);
    group_store_unnormalised<C>(pts, ztmp, n, i + half, group_neg<C>(add_mixed29<C>(T, q, true)), prod);
  }
  group_normalise_own<C>(pts, ztmp, n, i, half, 2, prod);
}

// out[bitrev(i)] = in[i]
template <class W>
static __global__ void group_bitrev_kernel(const Affine<W> *in, Affine<W> *out, int logn) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << logn)) return;
  copy_pod(out + (__brev(i) >> (32 - logn)), in + i);  // straight across: a local copy of a 128-byte point goes through the stack
}

// [e] P == O for every point, e the same for all of them: the order-r test of a vector of G2 points (e = r; the twist's cofactor
// has small factors, so a random combination would let a low-order component through with noticeable probability).  e is public
// and common: `naf`, `top` as group_uniform_mul reads them.  Infinity entries pass (the caller refuses them earlier).
template <class C>
static __global__ __launch_bounds__(GROUP_THREADS) void group_order_check_kernel(const Affine<typename C::W> *pts, uint32_t n, const uint32_t *naf, int top, uint32_t *bad) {
  const uint32_t i = blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (i >= n) return;
  const Affine<typename C::W> p = load_pod(pts + i);
  if (p.is_inf()) return;
  if (!group_uniform_mul<C>(group_affine_in<C>(p), naf, top).is_inf()) group_note_bad(bad, i);
}

// Every point satisfies its curve's equation y^2 = x^3 + b (Montgomery coordinates x 2^256, the key's wire form); infinity
// passes or fails as the caller says.
template <class F>
static __global__ void group_on_curve_kernel(const Affine<F> *pts, uint32_t n, F b, bool infinity_passes, uint32_t *bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = load_pod(pts + i);
  if (p.is_inf() ? infinity_passes : sqr(p.y) == add(mul(sqr(p.x), p.x), b)) return;
  group_note_bad(bad, i);
}
inline Fq group_curve_b(const Fq *) { return pairing::fq_small(3); }
inline Fq2 group_curve_b(const Fq2 *) { return Fq2{pairing::fq_from_limbs(pairing::TWIST_B0), pairing::fq_from_limbs(pairing::TWIST_B1)}; }
template <class F>
void group_on_curve_launch(const void *pts, uint32_t n, bool infinity_passes, uint32_t *bad) {
  group_on_curve_kernel<F><<<(n + 255) / 256, 256>>>((const Affine<F> *)pts, n, group_curve_b((const F *)nullptr), infinity_passes, bad);
}

// Sparse linear combinations of points: task t sums the terms [tb[t], tb[t + 1]) -- term e = coefficient x pts[row[e]] -- into
// out[dst[t]], one thread per task.  A coefficient c of a real circuit is almost always 1, r - 1 or small, so the host stores
// the shorter of c and r - c (`mag`, 8 words per term) with meta[e] = its bit length | sign << 31: a term of magnitude one is ONE
// mixed addition, any other a ladder of its own length and a full addition.  The host cuts columns into tasks of bounded work;
// the partial sums of a cut column are added by further launches of this kernel (row[e] then points into `out` itself).
template <class C>
static __global__ __launch_bounds__(GROUP_THREADS) void group_combine_kernel(Affine<typename C::W> *out, typename C::W *ztmp, size_t n_out, uint32_t n_tasks, const uint32_t *tb,
                                                                              const uint32_t *dst, const uint32_t *row, const uint32_t *meta, const uint32_t *mag,
                                                                              const Affine<typename C::W> *pts) {
  const uint32_t t = blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (t >= n_tasks) return;
  XYZZ29<C> acc = XYZZ29<C>::inf();
#pragma unroll 1
  for (uint32_t e = tb[t], end = tb[t + 1]; e < end; e++) {
    const Affine<typename C::W> p = load_pod(pts + row[e]);
    const uint32_t m = meta[e];
    const int bits = (int)(m & 0x1ffu);
    const bool minus = (m >> 31) != 0;
    if (p.is_inf() || bits == 0) continue;
    const Affine29<C> q = group_affine_in<C>(p);
    if (bits == 1) { acc = add_mixed29<C>(acc, q, minus); continue; }
    XYZZ29<C> T = group_lane_mul<C>(q, mag + 8 * (size_t)e, bits);
    if (minus) T = group_neg<C>(T);
    acc = add_full29<C>(acc, T);
  }
  auto prod = C::one().template to<4>();
  const size_t o = dst[t];
  group_store_unnormalised<C>(out, ztmp, n_out, o, acc, prod);
  group_normalise_own<C>(out, ztmp, n_out, o, 0, 1, prod);
}

// out[i] = a[i] - b[i] (hExps[i] = tau^(i+m) G - tau^i G); no entry of a or b is infinity
template <class C>
static __global__ __launch_bounds__(GROUP_THREADS) void group_diff_kernel(Affine<typename C::W> *out, const Affine<typename C::W> *a, const Affine<typename C::W> *b, uint32_t n,
                                                                           typename C::W *ztmp) {
  const uint32_t i = blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (i >= n) return;
  const Affine29<C> qa = group_affine_in<C>(load_pod(a + i)), qb = group_affine_in<C>(load_pod(b + i));
  auto prod = C::one().template to<4>();
  group_store_unnormalised<C>(out, ztmp, n, i, add_mixed29<C>(make_xyzz<C>(qa.x, qa.y, C::one(), C::one()), qb, true), prod);
  group_normalise_own<C>(out, ztmp, n, i, 0, 1, prod);
}

// out[o] = a[o] + b[i], o = dst[i] (dst null: o = i), for EVERY input: either side at infinity (under a shared support the `a`
// side is, for public signals and placeholders), both, P + P and P + (-P) (add_affine_affine29 has the last two).  An entry whose
// slot is outside the n_out points of `out` (RANK_NONE: the layout has no point for it) is skipped, and tallied in `bad` when its
// addend is finite.  The slots of a launch are distinct; out may be a.  ztmp: 2 n_out coordinates.
template <class C>
static __global__ __launch_bounds__(GROUP_THREADS) void group_add_each_kernel(Affine<typename C::W> *out, const Affine<typename C::W> *a, const Affine<typename C::W> *b, uint32_t n,
                                                                               const uint32_t *dst, uint32_t n_out, typename C::W *ztmp, uint32_t *bad) {
  const uint32_t i = blockIdx.x * GROUP_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = dst ? dst[i] : i;
  const Affine<typename C::W> pb = load_pod(b + i);
  if (o >= n_out) {
    if (!pb.is_inf()) group_note_bad(bad, i);
    return;
  }
  const Affine<typename C::W> pa = load_pod(a + o);
  XYZZ29<C> acc = XYZZ29<C>::inf();
  if (pa.is_inf() || pb.is_inf()) {
    if (!pa.is_inf() || !pb.is_inf()) {
      const Affine29<C> q = group_affine_in<C>(pa.is_inf() ? pb : pa);
      acc = make_xyzz<C>(q.x, q.y, C::one(), C::one());
    }
  } else {
    acc = add_affine_affine29<C>(group_affine_in<C>(pa), false, group_affine_in<C>(pb), false);
  }
  auto prod = C::one().template to<4>();
  group_store_unnormalised<C>(out, ztmp, n_out, o, acc, prod);
  group_normalise_own<C>(out, ztmp, n_out, o, 0, 1, prod);
}

// Infinity as the fixed-base setup writes it (the websnark wire form: x = 0, y = one) where the kernels above leave all zeros, so
// that a table derived from points is the bytes of the table made from scalars.
template <class W>
static __global__ void group_inf_wire_kernel(Affine<W> *pts, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (load_pod(&pts[i].x).is_zero()) store_pod(&pts[i].y, W::one());
}

// Montgomery -> standard form, in place (the ladders read plain bits)
static __global__ void fr_to_std_kernel(Fr *T, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  store_fr(T + k, from_mont(load_fr(T + k)));
}

}  // namespace zkr
