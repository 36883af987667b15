// host_arith_shim.cpp -- exposes the field/curve templates, compiled for the HOST, through a
// tiny C ABI so tests/test_host_arith.py can check them against the oracle without a GPU.
// Not part of the product path (the product is libzkr_hip.so).
// What the host build does NOT share with the device (field.hpp chooses by __HIP_DEVICE_COMPILE__): mul -- and so sqr, to_mont,
// from_mont, inv -- is mul_host64 here and the 96-bit column scan of the mac96* asm statements there; mul_sum2 / mul_sum4 add
// separate products here and are one fused scan there (field_fused.hpp); the Fq2 product is Karatsuba here and schoolbook through
// mul_sum2 there; both mul_sub go through those.  A pass of the tests of this shim says nothing about the device's side of these:
// zkt_fp_raw below and zkr_selftest_fp (zkr_selftest.hip) run ONE function, field_raw_op, in the two builds on raw edge limbs, and
// tests/test_field_raw_cpu.py / tests/test_gpu_field_raw.py compare each with integers and the two with each other.
#include "hostops.hpp"
#include "pairing.hpp"
#include "curve29.hpp"
#include "curve29_raw.hpp"
#include "field_raw.hpp"
#include "msm_plan.hpp"
#include "eval_h.hpp"
using namespace zkr;

// ---- the 29-bit-limb hot-path arithmetic (field29.hpp, curve29.hpp) compiled for the host
namespace {
template <class P29> L29<P29, 3> to_m261(const uint8_t *std32) {  // standard form -> x 2^261
  uint32_t w[8];
  memcpy(w, std32, 32);
  return mul(unpack29<P29, 10>(w), const29<P29>(P29::R2)).template to<3>();
}
template <class P29, int H> void from_m261(const L29<P29, H> &x, uint8_t *std32) {  // x 2^261 (any bound a product accepts) -> canonical standard form
  L29<P29, 2> raw_one = L29<P29, 2>::zero();
  raw_one.v[0] = 1;
  uint32_t w[8];
  pack29(canonical(mul(x, raw_one)), w);
  memcpy(std32, w, 32);
}
template <class P29> void f29_op(int op, const uint8_t *a32, const uint8_t *b32, uint8_t *out) {
  auto a = to_m261<P29>(a32), b = to_m261<P29>(b32);
  switch (op) {
    case 0: from_m261(mul(a, b), out); break;
    case 1: from_m261(sqr(a), out); break;
    case 2: from_m261(add(a, b), out); break;
    case 3: from_m261(sub(a, b), out); break;
    case 4: from_m261(neg(a), out); break;
    case 5: from_m261(mul_sub(a, b, b, a), out); break;                                  // 0
    case 6: from_m261(mul_sum2(a, a, b, b), out); break;                                 // a^2 + b^2
    case 7: {  // values at the wide end of their bounds: ((a - b) - (b - a) + 2 (a + b))^2 with lazy intermediates
      auto t = sub(sub(a, b), sub(b, a));                 // 2 (a - b), bound 3 + 4 + 8 = 15 half moduli
      auto u = add(t, dbl(add(a, b)));                    // + 2 (a + b): 4 a, bound 15 + 12 = 27... too wide for a square: reduce
      from_m261(sqr(weak(u)), out);                       // 16 a^2
      break;
    }
    case 8: from_m261(mul_sum4(a, b, a, a, b, b, neg(a), b), out); break;               // a b + a^2 + b^2 - a b
    case 9: from_m261(weak(sub(sub(sub(a, b), b), b)), out); break;                      // a - 3 b through three lazy subtractions
    case 11: from_m261(mul(a, neg_loose(b)), out); break;                                 // -a b, the negation without its carry sweep
    case 12: from_m261(mul(b, sub_loose(a, b)), out); break;                              // b (a - b)
    case 13: from_m261(mul_sum2(a, sub_loose(a, b), neg_loose(b), a), out); break;        // a (a - b) - a b: the shape of the Y coordinate
    case 14: from_m261(mul_cneg(a, true, b), out); break;                                 // -a b through the per-lane sign select
    case 15: from_m261(mul_cneg(a, false, b), out); break;                                // a b
    default: from_m261(mul(sub(a, b).template to<17>(), sub(b, a).template to<17>()), out);  // -(a - b)^2 at the widest bound the group law uses
  }
}
}  // namespace

// sum_i (+-) P_i with the hot-path group law: points in the key's wire form (affine, x 2^256; 64 B G1 / 128 B G2), signs[i] != 0
// subtracts.  The list is cut in two halves that are accumulated apart (add_mixed29) and then added (add_full29); with
// `twice` the total is added to itself (the doubling branch of add_full29).  out: standard-form affine; returns 1 for infinity.
template <class F> static int chain29(const uint8_t *pts, const uint8_t *signs, size_t n, int twice, uint8_t *out) {
  using C = typename CoordOf<F>::C;
  const size_t pb = sizeof(Affine<F>);
  XYZZ29<C> half[2] = {XYZZ29<C>::inf(), XYZZ29<C>::inf()};
  for (size_t i = 0; i < n; i++) {
    Affine<F> p;
    memcpy(&p, pts + i * pb, pb);
    if (p.is_inf()) continue;
    Affine<F> q{radix_to_261(p.x), radix_to_261(p.y)};
    XYZZ29<C> &acc = half[i >= n / 2];
    acc = add_mixed29<C>(acc, unpack_affine(q), signs[i] != 0);
    acc = unpack_xyzz(pack_xyzz<F>(acc));   // through the packed form, as the kernels store buckets
  }
  XYZZ29<C> tot = add_full29<C>(half[0], half[1]);
  if (twice) tot = add_full29<C>(tot, unpack_xyzz(pack_xyzz<F>(tot)));
  XYZZ<F> res = xyzz_to_256(pack_xyzz<F>(tot));
  if (res.is_inf()) return 1;
  Affine<F> a = to_affine(res);
  if constexpr (sizeof(F) == 32) store_g1_std(out, *reinterpret_cast<G1Affine *>(&a));
  else store_g2_std(out, *reinterpret_cast<G2Affine *>(&a));
  return 0;
}
// sum_i (+-) P_i as the accumulation kernels walk a fresh chain (kernels_msm.hpp chain_head, msm_accum_kernel): the first two
// entries through add_affine_affine29 -- an infinity placeholder among them leaves at most one point, which starts the chain --
// and the rest through add_mixed29.  Points, signs and result as chain29.
template <class F> static int chain29_from_head(const uint8_t *pts, const uint8_t *signs, size_t n, uint8_t *out) {
  using C = typename CoordOf<F>::C;
  const size_t pb = sizeof(Affine<F>);
  std::vector<Affine<F>> q(n);
  for (size_t i = 0; i < n; i++) {
    memcpy(&q[i], pts + i * pb, pb);
    if (!q[i].is_inf()) q[i] = Affine<F>{radix_to_261(q[i].x), radix_to_261(q[i].y)};
  }
  XYZZ29<C> acc = XYZZ29<C>::inf();
  size_t j = 0;
  if (n >= 2) {
    if (!q[0].is_inf() && !q[1].is_inf()) acc = add_affine_affine29<C>(unpack_affine(q[0]), signs[0] != 0, unpack_affine(q[1]), signs[1] != 0);
    else if (!q[0].is_inf()) acc = add_mixed29<C>(acc, unpack_affine(q[0]), signs[0] != 0);
    else if (!q[1].is_inf()) acc = add_mixed29<C>(acc, unpack_affine(q[1]), signs[1] != 0);
    j = 2;
  }
  for (; j < n; j++)
    if (!q[j].is_inf()) acc = add_mixed29<C>(acc, unpack_affine(q[j]), signs[j] != 0);
  XYZZ<F> res = xyzz_to_256(pack_xyzz<F>(acc));   // through the packed form, as the kernels store buckets
  if (res.is_inf()) return 1;
  Affine<F> a = to_affine(res);
  if constexpr (sizeof(F) == 32) store_g1_std(out, *reinterpret_cast<G1Affine *>(&a));
  else store_g2_std(out, *reinterpret_cast<G2Affine *>(&a));
  return 0;
}
// 2^(c l) P for l = 1..levels as msm_precompute_kernel computes them: Jacobian doubling chain on the 29-bit limbs, ONE
// inversion of the product of the denominators, affine results.  p: wire form (x 2^256); out: levels x standard-form affine
template <class F> static void jac_levels29(const uint8_t *pt, int c, int levels, uint8_t *out) {
  using C = typename CoordOf<F>::C;
  Affine<F> p;
  memcpy(&p, pt, sizeof p);
  p.x = radix_to_261(p.x); p.y = radix_to_261(p.y);
  Jac29<C> q{C::template unpack<2>(p.x).template to<JX>(), C::template unpack<2>(p.y).template to<JY>(), C::one().template to<JZ>()};
  std::vector<Jac29<C>> lv;
  auto prod = C::one().template to<4>();
  for (int l = 0; l < levels; l++) {
    for (int b = 0; b < c; b++) q = dbl_jac29<C>(q);
    lv.push_back(q);
    prod = mul(prod, q.z).template to<4>();
  }
  auto inv = inv29(prod);
  for (int l = levels - 1; l >= 0; l--) {
    auto pre = C::one().template to<4>();
    for (int j = 0; j < l; j++) pre = mul(pre, lv[j].z).template to<4>();
    auto iz = mul(inv, pre);
    inv = mul(inv, lv[l].z).template to<4>();
    auto iz2 = sqr(iz);
    auto iz3 = mul(iz2, iz);
    Affine<F> a{radix_to_256(C::template pack<2>(canonical_small(mul(lv[l].x, iz2)))), radix_to_256(C::template pack<2>(canonical_small(mul(lv[l].y, iz3))))};
    if constexpr (sizeof(F) == 32) store_g1_std(out + (size_t)l * 64, *reinterpret_cast<G1Affine *>(&a));
    else store_g2_std(out + (size_t)l * 128, *reinterpret_cast<G2Affine *>(&a));
  }
}

// ---- the chain-head and running-sum forms of curve29.hpp on coordinates given as integers (standard form, 32 B per Fq word; an Fq2
// coordinate is re, im).  The forms are arithmetic identities, so the tests feed them coordinates at the edges of their bounds as
// well as points of the curve.
template <class C> struct CoordIO;
template <> struct CoordIO<G1C> {
  static constexpr size_t bytes = 32;
  static L29<Fq29, 2> in(const uint8_t *p) { return canonical(to_m261<Fq29>(p)); }
  template <int H> static void out(const L29<Fq29, H> &x, uint8_t *p) { from_m261(x, p); }
};
template <> struct CoordIO<G2C> {
  static constexpr size_t bytes = 64;
  static Q29<2> in(const uint8_t *p) { return Q29<2>{canonical(to_m261<Fq29>(p)), canonical(to_m261<Fq29>(p + 32))}; }
  template <int H> static void out(const Q29<H> &x, uint8_t *p) { from_m261(x.a, p); from_m261(x.b, p + 32); }
};
template <class C> static int xyzz_out(const XYZZ29<C> &r, uint8_t *out) {  // X, Y, ZZ, ZZZ; 1 for infinity
  using IO = CoordIO<C>;
  if (r.is_inf()) return 1;
  IO::out(weak(r.x), out); IO::out(r.y, out + IO::bytes); IO::out(r.zz, out + 2 * IO::bytes); IO::out(r.zzz, out + 3 * IO::bytes);
  return 0;
}
// (+-a) + (+-b) of two affine points (x, y each) through add_affine_affine29
template <class C> static int affine_affine29(const uint8_t *a, int neg_a, const uint8_t *b, int neg_b, uint8_t *out) {
  using IO = CoordIO<C>;
  Affine29<C> pa{IO::in(a), IO::in(a + IO::bytes)}, pb{IO::in(b), IO::in(b + IO::bytes)};
  return xyzz_out<C>(add_affine_affine29<C>(pa, neg_a != 0, pb, neg_b != 0), out);
}

// the group law on raw limbs (curve29_raw.hpp), one operation over n records
template <class C, int OP> static void curve_raw_run(const uint32_t *records, size_t n, uint32_t *out, uint8_t *inf) {
  constexpr int RW = curve29_record_words(Raw29<C>::g2, OP), OW = curve29_out_words(Raw29<C>::g2, OP);
  for (size_t i = 0; i < n; i++) curve29_raw_op<C, OP>(records + i * RW, out + i * OW, inf + i);
}
template <class C> static void curve_raw(int op, const uint32_t *records, size_t n, uint32_t *out, uint8_t *inf) {
  switch (op) {
    case 0: curve_raw_run<C, 0>(records, n, out, inf); break;
    case 1: curve_raw_run<C, 1>(records, n, out, inf); break;
    case 2: curve_raw_run<C, 2>(records, n, out, inf); break;
    case 3: curve_raw_run<C, 3>(records, n, out, inf); break;
    case 4: curve_raw_run<C, 4>(records, n, out, inf); break;
    case 5: curve_raw_run<C, 5>(records, n, out, inf); break;
    default: curve_raw_run<C, 6>(records, n, out, inf);
  }
}

#include <atomic>
#include <thread>
#include "shard_group.hpp"

// ShardGroup on the host: `parts` threads meet at `rounds` barriers; thread `fail_part` (if < parts) aborts the group instead of
// arriving at barrier `fail_round`.  Returns 0 when every thread saw what it must: all barriers passed in step (nobody a
// round ahead), or -- with a failure -- every thread returned false at or after the failing round and none hung.
static int shard_group_selftest(unsigned parts, unsigned rounds, unsigned fail_part, unsigned fail_round) {
  zkr::ShardGroup g;
  g.parts = parts;
  g.vecs.resize(parts);
  std::vector<std::atomic<unsigned>> at(parts);
  for (auto &a : at) a.store(0);
  std::atomic<int> bad{0};
  auto work = [&](unsigned i) {
    for (unsigned r = 0; r < rounds; r++) {
      if (i == fail_part && r == fail_round) { g.abort(); return; }
      at[i].store(r + 1);
      const bool ok = g.barrier();
      if (!ok) { if (fail_part >= parts || r < fail_round) bad++; return; }  // a refusal without (or before) the failure
      for (unsigned j = 0; j < parts; j++)
        if (at[j].load() < r + 1) bad++;                                     // somebody had not arrived: the barrier let us through early
    }
    if (fail_part < parts && fail_round < rounds) bad++;                     // ran to the end although a shard failed
  };
  std::vector<std::thread> thr;
  for (unsigned i = 1; i < parts; i++) thr.emplace_back(work, i);
  work(0);
  for (auto &t : thr) t.join();
  return bad.load();
}

// ShardGroup::unsatisfied on the host: `parts` threads meet at a barrier, then each writes its count (counts[part]) as a shard's
// thread does when it collects its proof; the sum is taken after the threads have joined.  Returns the sum, or ~0 when a thread was
// refused at the barrier.
static unsigned long long shard_group_count_selftest(unsigned parts, const unsigned *counts) {
  zkr::ShardGroup g;
  g.parts = parts;
  g.vecs.resize(parts);
  g.unsatisfied.assign(parts, 0);
  std::atomic<int> bad{0};
  auto work = [&](unsigned i) {
    if (!g.barrier()) { bad++; return; }
    g.unsatisfied[i] = counts[i];
  };
  std::vector<std::thread> thr;
  for (unsigned i = 1; i < parts; i++) thr.emplace_back(work, i);
  work(0);
  for (auto &t : thr) t.join();
  return bad.load() ? ~0ull : g.unsatisfied_sum();
}

extern "C" {
unsigned long long zkr_host_shard_group_count_selftest(unsigned parts, const unsigned *counts) { return shard_group_count_selftest(parts, counts); }
// msm_plan(n_scalars, n_points, c_fixed) as ten words: c, K, glog, nbw, nb, big_thresh, nR, nbl, J, S
void zkt_msm_plan(size_t n_scalars, size_t n_points, int c_fixed, uint32_t out[10]) {
  const MsmPlan p = msm_plan(n_scalars, n_points, c_fixed);
  const uint32_t w[10] = {(uint32_t)p.c, (uint32_t)p.K, (uint32_t)p.glog, p.nbw, p.nb, p.big_thresh, p.nR, p.nbl, p.J, p.S};
  memcpy(out, w, sizeof w);
}
uint32_t zkt_big_threshold(size_t n_points, int K, uint32_t nbw, int nbat) { return big_threshold(n_points, K, nbw, nbat); }
// proof_layout of a key with n witness scalars, m scalars of h, npts[t] points and window win_c[t] (0: the plan's own) per table, as a
// key plans its tables (zkr_key.hip key_alloc_workspace).  out, 63 ints: share_b, share_ac, n_chains, then per table (5 x)
// sort_src, chain, set, flags, own_result, then per chain (5 x, unused ones as the layout leaves them) n_members, members[2], sets,
// geom, g2, latency.  Returns 1 when same_reduce_geometry(A, B1).
int zkt_proof_layout(uint32_t n, uint32_t m, const uint32_t npts[5], const uint32_t win_c[5], int share_b, int share_ac, int out[63]) {
  MsmPlan plan[N_TABLES];
  for (int t = 0; t < N_TABLES; t++) plan[t] = msm_plan(t == T_H ? m : n, npts[t], (int)win_c[t]);
  const ProofLayout L = proof_layout(npts, share_b != 0, share_ac != 0, plan);
  int *o = out;
  *o++ = L.share_b; *o++ = L.share_ac; *o++ = L.n_chains;
  for (int t = 0; t < N_TABLES; t++) { *o++ = L.sort_src[t]; *o++ = L.chain[t]; *o++ = L.set[t]; *o++ = L.flags[t]; *o++ = L.own_result(t); }
  for (const ChainLayout &c : L.chains) { *o++ = c.n_members; *o++ = c.members[0]; *o++ = c.members[1]; *o++ = c.sets; *o++ = c.geom; *o++ = c.g2; *o++ = c.latency; }
  return same_reduce_geometry(plan[T_A], plan[T_B1]);
}
int zkr_host_shard_group_selftest(unsigned parts, unsigned rounds, unsigned fail_part, unsigned fail_round) {
  return shard_group_selftest(parts, rounds, fail_part, fail_round);
}
// eval_h.hpp: host_ntt on 2^logn standard-form values in place (natural order in and out)
void zkt_host_ntt(uint8_t *data, unsigned logn, int inverse) {
  std::vector<Fr> x((size_t)1 << logn);
  for (size_t i = 0; i < x.size(); i++) x[i] = to_mont(load_fp<FrParams>(data + 32 * i));
  host_ntt(x, logn, inverse != 0);
  for (size_t i = 0; i < x.size(); i++) store_fp(data + 32 * i, from_mont(x[i]));
}
// eval_h.hpp: eval_h_scalars with every value in standard form, 32 B each (hx, f, e, eprime: 2^logm; coefC: one per term of C;
// cpriv: n - p - 1; cfold: n)
void zkt_eval_h_scalars(const uint8_t *hx, unsigned logm, const uint32_t *rowC, const uint32_t *sigC, const uint8_t *coefC, uint32_t nC, uint32_t n, uint32_t p,
                        const uint8_t *cpriv, uint8_t *f, uint8_t *e, uint8_t *cfold, uint8_t *eprime) {
  auto load = [](const uint8_t *b, size_t cnt) {
    std::vector<Fr> v(cnt);
    for (size_t i = 0; i < cnt; i++) v[i] = to_mont(load_fp<FrParams>(b + 32 * i));
    return v;
  };
  auto store = [](const std::vector<Fr> &v, uint8_t *b) {
    for (size_t i = 0; i < v.size(); i++) store_fp(b + 32 * i, from_mont(v[i]));
  };
  const std::vector<Fr> vhx = load(hx, (size_t)1 << logm), vco = load(coefC, rowC[nC]), vcp = load(cpriv, n - p - 1);
  EvalHScalars sc;
  eval_h_scalars(vhx.data(), logm, rowC, sigC, vco.data(), nC, n, p, vcp.data(), sc);
  store(sc.f, f); store(sc.e, e); store(sc.cfold, cfold); store(sc.eprime, eprime);
}
// field 0 = Fq, 1 = Fr; ops: see f29_op above; inputs / outputs standard form
void zkt29_fp(int field, int op, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  if (field == 0) f29_op<Fq29>(op, a, b, out); else f29_op<Fr29>(op, a, b, out);
}
// pack / unpack round trip and the change of radix both ways on a raw 256-bit word string (x 2^256 form in, same out)
void zkt29_radix_roundtrip(const uint8_t *in32, uint8_t *out32, uint8_t *mid32) {
  Fq w;
  memcpy(w.v, in32, 32);
  Fq m = radix_to_261(w);
  memcpy(mid32, m.v, 32);
  Fq back = radix_to_256(m);
  memcpy(out32, back.v, 32);
}
// the four product forms on raw limbs (field29.hpp f29_raw_form, host build = the defining recursion); layout as
// zkr_selftest_f29_forms
void zkt29_raw_forms(int field, int form, const uint32_t *records, size_t n, uint32_t *out) {
  for (size_t i = 0; i < n; i++) {
    uint32_t op[8][9], r[9];
    memcpy(op, records + i * 72, sizeof op);
    if (field == 0) f29_raw_form<Fq29>(form, op, r); else f29_raw_form<Fr29>(form, op, r);
    memcpy(out + i * 9, r, sizeof r);
  }
}
// barrett() and canonical_small() of field29.hpp on raw limbs: in = 9 limbs (low eight below 2^29, value below 64 p),
// out = 9 limbs of barrett(in), canon = 9 limbs of canonical_small(barrett(in))
void zkt29_barrett(int field, const uint32_t *in, uint32_t *out, uint32_t *canon) {
  if (field == 0) {
    L29<Fq29, 128> a; memcpy(a.v, in, 36);
    auto b = barrett(a); memcpy(out, b.v, 36);
    auto c = canonical_small(b); memcpy(canon, c.v, 36);
  } else {
    L29<Fr29, 128> a; memcpy(a.v, in, 36);
    auto b = barrett(a); memcpy(out, b.v, 36);
    auto c = canonical_small(b); memcpy(canon, c.v, 36);
  }
}
// the sweep-less differences on raw limbs (a, b: 9 normalised limbs, value below 13 / 4 half moduli as the accumulator's X / Y
// are): nl = neg_loose(b), sl = sub_loose(a, b) as limbs, for the range and value checks of tests/test_host_arith.py
void zkt29_loose(int field, const uint32_t *a9, const uint32_t *b9, uint32_t *nl, uint32_t *sl, int *k_neg, int *k_sub) {
  if (field == 0) {
    L29<Fq29, 4> a; L29<Fq29, 13> b; memcpy(a.v, a9, 36); memcpy(b.v, b9, 36);
    auto n = neg_loose(b); auto d = sub_loose(a, b);
    memcpy(nl, n.v, 36); memcpy(sl, d.v, 36); *k_neg = decltype(n)::bound / 2; *k_sub = (decltype(d)::bound - 4) / 2;
  } else {
    L29<Fr29, 4> a; L29<Fr29, 13> b; memcpy(a.v, a9, 36); memcpy(b.v, b9, 36);
    auto n = neg_loose(b); auto d = sub_loose(a, b);
    memcpy(nl, n.v, 36); memcpy(sl, d.v, 36); *k_neg = decltype(n)::bound / 2; *k_sub = (decltype(d)::bound - 4) / 2;
  }
}
// the group law of curve29.hpp on raw limbs, nothing reduced on the way in or out: records, operations and results as
// curve29_raw.hpp lays them out (and as zkr_selftest_curve29 runs them on the device); inf[i] = 1 for the point at infinity
void zkt29_curve_raw(int g2, int op, const uint32_t *records, size_t n, uint32_t *out, uint8_t *inf) {
  if (g2) curve_raw<G2C>(op, records, n, out, inf); else curve_raw<G1C>(op, records, n, out, inf);
}
// the bounds (half moduli) the register forms of curve29.hpp declare: HX, HY, JX, JY, JZ
void zkt29_curve_bounds(int out[5]) {
  const int b[5] = {HX, HY, JX, JY, JZ};
  memcpy(out, b, sizeof b);
}
void zkt29_g1_levels(const uint8_t *pt, int c, int levels, uint8_t *out) { jac_levels29<Fq>(pt, c, levels, out); }
void zkt29_g2_levels(const uint8_t *pt, int c, int levels, uint8_t *out) { jac_levels29<Fq2>(pt, c, levels, out); }
int zkt29_affine_affine(int g2, const uint8_t *a, int neg_a, const uint8_t *b, int neg_b, uint8_t *out) {
  return g2 ? affine_affine29<G2C>(a, neg_a, b, neg_b, out) : affine_affine29<G1C>(a, neg_a, b, neg_b, out);
}
int zkt29_chain_from_head(int g2, const uint8_t *pts, const uint8_t *signs, size_t n, uint8_t *out) {
  return g2 ? chain29_from_head<Fq2>(pts, signs, n, out) : chain29_from_head<Fq>(pts, signs, n, out);
}
int zkt29_g1_chain(const uint8_t *pts, const uint8_t *signs, size_t n, int twice, uint8_t *out) { return chain29<Fq>(pts, signs, n, twice, out); }
int zkt29_g2_chain(const uint8_t *pts, const uint8_t *signs, size_t n, int twice, uint8_t *out) { return chain29<Fq2>(pts, signs, n, twice, out); }

// the 8 x 32-bit-limb field on raw limbs, nothing converted on the way in or out: records (n x 64 words), operations and results
// (n x 8 words, the Fq2 ops 16) as field_raw.hpp lays them out and as zkr_selftest_fp runs them on the device.  field 0 = Fq,
// 1 = Fr; a pair (field, op) that field_raw_valid refuses writes nothing
void zkt_fp_raw(int field, int op, const uint32_t *records, size_t n, uint32_t *out) {
  if (!field_raw_valid(field, op)) return;
  const size_t ow = (size_t)field_raw_out_words(op);
  auto run = [&](auto pm) {
    using PM = decltype(pm);
    field_raw_dispatch<PM>(op, [&](auto tag) {
      for (size_t i = 0; i < n; i++) field_raw_op<PM, decltype(tag)::value>(records + i * FIELD_RAW_RECORD_WORDS, out + i * ow);
    });
  };
  if (field) run(FrParams{}); else run(FqParams{});
}
// op: 0 mul, 1 add, 2 sub, 3 inv(a), 4 neg(a), 5 sqr(a); inputs/outputs standard form
void zkt_fp(int field, int op, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  if (field == 0) {
    Fq x = to_mont(load_fp<FqParams>(a)), y = to_mont(load_fp<FqParams>(b)), r;
    switch (op) { case 0: r = mul(x, y); break; case 1: r = add(x, y); break; case 2: r = sub(x, y); break;
                  case 3: r = inv(x); break; case 4: r = neg(x); break; default: r = sqr(x); }
    store_fp(out, from_mont(r));
  } else {
    Fr x = to_mont(load_fp<FrParams>(a)), y = to_mont(load_fp<FrParams>(b)), r;
    switch (op) { case 0: r = mul(x, y); break; case 1: r = add(x, y); break; case 2: r = sub(x, y); break;
                  case 3: r = inv(x); break; case 4: r = neg(x); break; default: r = sqr(x); }
    store_fp(out, from_mont(r));
  }
}
// a, b: 64 B standard (re, im); op 0 mul, 1 sqr(a), 2 inv(a)
void zkt_fq2(int op, const uint8_t *a, const uint8_t *b, uint8_t *out) {
  Fq2 x{to_mont(load_fp<FqParams>(a)), to_mont(load_fp<FqParams>(a + 32))};
  Fq2 y{to_mont(load_fp<FqParams>(b)), to_mont(load_fp<FqParams>(b + 32))};
  Fq2 r = op == 0 ? mul(x, y) : op == 1 ? sqr(x) : inv(x);
  store_fp(out, from_mont(r.a));
  store_fp(out + 32, from_mont(r.b));
}
// k*P with mixed adds only (exercises add_mixed incl. its doubling branch) -> std affine; returns 1 if infinity
int zkt_g1_mul(const uint8_t *p_mont, const uint8_t *k32, uint8_t *out) {
  G1Affine p = load_g1(p_mont);
  U256 k = load_u256(k32);
  G1XYZZ acc = G1XYZZ::inf();
  for (int i = 255; i >= 0; i--) {
    acc = dbl_xyzz(acc);
    if ((k.v[i >> 5] >> (i & 31)) & 1) acc = add_mixed(acc, p);
  }
  if (acc.is_inf()) return 1;
  store_g1_std(out, to_affine(acc));
  return 0;
}
int zkt_g2_mul(const uint8_t *p_mont, const uint8_t *k32, uint8_t *out) {
  G2Affine p = load_g2(p_mont);
  U256 k = load_u256(k32);
  G2XYZZ acc = scalar_mul(to_xyzz(p), k);
  if (acc.is_inf()) return 1;
  store_g2_std(out, to_affine(acc));
  return 0;
}
// (a*P) + (b*P) through add_full / add_mixed(neg) corner cases: returns std affine of a*P + sign*b*P
int zkt_g1_lincomb(const uint8_t *p_mont, uint32_t a, uint32_t b, int negate_b, uint8_t *out) {
  G1Affine p = load_g1(p_mont);
  G1XYZZ pa = mul_small(to_xyzz(p), a), pb = mul_small(to_xyzz(p), b);
  G1XYZZ r;
  if (!pb.is_inf()) {
    G1Affine qb = to_affine(pb);
    r = add_mixed(pa, qb, negate_b != 0);
  } else {
    r = pa;
  }
  if (r.is_inf()) return 1;
  store_g1_std(out, to_affine(r));
  return 0;
}
// The verifier's structured final exponentiation (Frobenius maps + three powers by x) against plain square-and-multiply
// over (q^12 - 1)/r, and the Frobenius maps against powers by q, on `count` pseudo-random Fq12 elements (xorshift from
// `seed`).  Returns the number of elements on which everything agrees.
int zkt_final_exp_check(uint64_t seed, int count) {
  using namespace zkr::pairing;
  uint64_t st = seed ? seed : 88172645463325252ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); };
  auto rfq = [&]() { Fq a; for (int i = 0; i < 8; i++) a.v[i] = rnd(); a.v[7] &= 0x0fffffffu; return to_mont(a); };
  auto rfq2 = [&]() { Fq2 r; r.a = rfq(); r.b = rfq(); return r; };
  auto rfq6 = [&]() { Fq6 r; r.c0 = rfq2(); r.c1 = rfq2(); r.c2 = rfq2(); return r; };
  uint32_t q[8];
  for (int i = 0; i < 8; i++) q[i] = FqParams::P[i];
  int ok = 0;
  for (int it = 0; it < count; it++) {
    Fq12 f{rfq6(), rfq6()};
    Fq12 fq = pow(f, q);
    ok += (fq == frobenius(f)) && (pow(fq, q) == frobenius2(f)) && (final_exponentiation_plain(f) == final_exponentiation(f));
  }
  return ok;
}
// The verifier's inversion-free Miller loop (projective steps for arbitrary second arguments, prepared lines for fixed ones)
// against the affine loop, after the final exponentiation: `count` rounds of three pairs (a_i G1, b_i G2) with pseudo-random
// small multiples of the generators (g1 64 B, g2 128 B standard form), every split of the pairs into "arbitrary" and "prepared",
// one pair with a point at infinity in the last round.  Returns the number of agreeing comparisons (count * 4 expected).
int zkt_miller_loops_agree(const uint8_t *g1, const uint8_t *g2, uint64_t seed, int count) {
  using namespace zkr::pairing;
  uint64_t st = seed ? seed : 88172645463325252ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 16); };
  G1Affine P{to_mont(load_fp<FqParams>(g1)), to_mont(load_fp<FqParams>(g1 + 32))};
  G2Affine Q{Fq2{to_mont(load_fp<FqParams>(g2)), to_mont(load_fp<FqParams>(g2 + 32))}, Fq2{to_mont(load_fp<FqParams>(g2 + 64)), to_mont(load_fp<FqParams>(g2 + 96))}};
  auto g2_mul = [&](uint32_t k) {
    G2XYZZ acc = G2XYZZ::inf();
    for (int b = 31; b >= 0; b--) { acc = dbl_xyzz(acc); if ((k >> b) & 1) acc = add_mixed(acc, Q); }
    return to_affine(acc);
  };
  int agree = 0;
  for (int it = 0; it < count; it++) {
    G1Affine ps[3];
    G2Affine qs[3];
    for (int i = 0; i < 3; i++) {
      ps[i] = to_affine(mul_small(to_xyzz(P), (rnd() & 0xffff) + 1));
      qs[i] = g2_mul((rnd() & 0xfffff) + 1);
    }
    if (it == count - 1) ps[1] = G1Affine{Fq::zero(), Fq::one()};  // infinity as the wire form has it: the pair contributes 1
    bool ok = true;
    const Fq12 want = final_exponentiation(multi_miller_loop(ps, qs, 3, &ok));
    if (!ok) continue;
    for (int nfixed = 0; nfixed <= 3; nfixed++) {  // the last nfixed pairs prepared
      G2Prepared prep[3];
      const G2Prepared *pp[3];
      bool good = true;
      for (int j = 0; j < nfixed; j++) { good = g2_prepare(qs[3 - nfixed + j], prep[j]) && good; pp[j] = &prep[j]; }
      bool ok2 = true;
      const Fq12 got = final_exponentiation(miller_loop_mixed(ps, qs, 3 - nfixed, ps + 3 - nfixed, pp, nfixed, &ok2));
      agree += good && ok2 && got == want;
    }
  }
  return agree;
}
// The host twin of zkr_pairing_device (include/zkr.h): e(P_i, Q_i) after the final exponentiation through the header code the
// device kernel runs (miller_loop_proj, final_exponentiation with an explicit Consts), same input and output layout: g1 n x 64 B,
// g2 n x 128 B standard form (an all-zero point: infinity -> one), out n x 384 B, the twelve coefficients in the tower's order.
int zkt_pairing(const uint8_t *g1, const uint8_t *g2, size_t n, uint8_t *out, uint8_t *degenerate) {
  using namespace zkr::pairing;
  const Consts &k = host_consts();
  for (size_t i = 0; i < n; i++) {
    const uint8_t *a = g1 + 64 * i, *b = g2 + 128 * i;
    G1Affine P{to_mont(load_fp<FqParams>(a)), to_mont(load_fp<FqParams>(a + 32))};
    G2Affine Q{Fq2{to_mont(load_fp<FqParams>(b)), to_mont(load_fp<FqParams>(b + 32))}, Fq2{to_mont(load_fp<FqParams>(b + 64)), to_mont(load_fp<FqParams>(b + 96))}};
    bool ok = true;
    const Fq12 e = final_exponentiation(miller_loop_proj(P, Q, k, &ok), k);
    const Fq2 *co[6] = {&e.c0.c0, &e.c0.c1, &e.c0.c2, &e.c1.c0, &e.c1.c1, &e.c1.c2};
    for (int t = 0; t < 6; t++) {
      store_fp(out + 384 * i + 64 * t, from_mont(co[t]->a));
      store_fp(out + 384 * i + 64 * t + 32, from_mont(co[t]->b));
    }
    if (degenerate) degenerate[i] = ok ? 0 : 1;
  }
  return 0;
}
// the two G2 membership tests on one twist point (128 B standard form: x.re, x.im, y.re, y.im): bit 0 = the definition
// ([r]Q == infinity), bit 1 = the endomorphism test the verifier runs (psi(Q) == [6x^2]Q), bit 2 = the point is on the twist
int zkt_g2_membership(const uint8_t *pt) {
  using namespace zkr::pairing;
  G2Affine q{Fq2{to_mont(load_fp<FqParams>(pt)), to_mont(load_fp<FqParams>(pt + 32))}, Fq2{to_mont(load_fp<FqParams>(pt + 64)), to_mont(load_fp<FqParams>(pt + 96))}};
  return (g2_in_subgroup_plain(q) ? 1 : 0) | (g2_in_subgroup(q) ? 2 : 0) | (g2_on_curve(q) ? 4 : 0);
}
// proof-assembly helpers (hostops.hpp) against plain double-and-add: fixed-base window table, joint double
// multiplication; scalars a, b standard 32 B.  Returns 1 when both agree.
int zkt_assembly_muls(const uint8_t *p_mont, const uint8_t *q_mont, const uint8_t *a32, const uint8_t *b32) {
  G1Affine p = load_g1(p_mont), q = load_g1(q_mont);
  U256 a = load_u256(a32), b = load_u256(b32);
  G1XYZZ want_fixed = scalar_mul(to_xyzz(p), a);
  G1XYZZ got_fixed = fixed_base_mul(fixed_base_table(p), a);
  G1XYZZ want_joint = add_full(scalar_mul(to_xyzz(p), a), scalar_mul(to_xyzz(q), b));
  G1XYZZ got_joint = double_scalar_mul(to_xyzz(p), a, to_xyzz(q), b);
  auto same = [](const G1XYZZ &x, const G1XYZZ &y) {
    if (x.is_inf() || y.is_inf()) return x.is_inf() == y.is_inf();
    G1Affine u = to_affine(x), v = to_affine(y);
    return u.x == v.x && u.y == v.y;
  };
  return same(want_fixed, got_fixed) && same(want_joint, got_joint);
}
}
