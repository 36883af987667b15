// zkr_eval_tables.hip -- the side tables of H in evaluation form (zkr_internal.hpp EvalTables; the algebra: eval_h.hpp) for ANY
// whole key, derived from the key's own points.  zkr_setup.hip key_build_eval_tables makes them from the setup's scalars, which only
// a test or benchmark setup knows; a key loaded from websnark bytes or a file, a transcript key and every contributed key hold the
// same information as points, and both tables are linear images of those:
//     E'_j = ke 1/m sum_i (g w^j)^(-i) H_i      ke = -1/2 R / m^2 (eval_h.hpp eprime), H_i the key's hExps, g = w_2m
//     F_j  =    1/m sum_i w^(-ij) H_i
//     C'_s = C_s + 1/2 sum_j C_js F_j           every signal, the public ones too; C_s = infinity up to nPublic
// So: H_i times ke g^(-i), one inverse NTT over points; H_i times 1/2, one inverse NTT, one sparse combination over the columns of
// the circuit's C side, and the key's own C points added slot by slot.  The launches are the transcript setup's (zkr_ptau.hip,
// kernels_group.hpp); the per-slot addition is the one kernel made for this.  Affine canonical points are unique and the window
// levels are a function of level 0, so a derived table is the bytes of the table the scalar-knowing setup builds
// (zkr_key_eval_tables_equal).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "eval_h.hpp"
#include "kernels_group.hpp"
#include "zkr_internal.hpp"

namespace zkr {
namespace {

int refuse_in_flight(zkr_key *k, const char *what) {  // under k->mu
  for (const ProofSlot &sl : k->slot)
    if (sl.busy) { set_error("%s: the key has a proof in flight; collect it first", what); return ZKR_ERR_ARG; }
  return 0;
}

// `a + b -> out`, one launch; dst, n_out, bad as group_add_each_kernel takes them
template <class C>
int add_each_launch(Affine<typename C::W> *out, const Affine<typename C::W> *a, const Affine<typename C::W> *b, size_t n, const uint32_t *dst, size_t n_out, void *ztmp,
                    uint32_t *bad) {
  if (!n) return 0;
  group_add_each_kernel<C><<<(unsigned)((n + GROUP_THREADS - 1) / GROUP_THREADS), GROUP_THREADS>>>(out, a, b, (uint32_t)n, dst, (uint32_t)n_out, (typename C::W *)ztmp, bad);
  ZKR_HIP_CHECK(hipGetLastError());
  return 0;
}

template <class C>
int add_each_hook(void *points_mont, const void *addends_mont, size_t n) {
  using W = typename C::W;
  DevBuf pts, add, ztmp;
  int rc;
  if ((rc = pts.alloc(n * sizeof(Affine<W>))) || (rc = add.alloc(n * sizeof(Affine<W>))) || (rc = ztmp.alloc(2 * n * sizeof(W)))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(pts.p, points_mont, n * sizeof(Affine<W>), hipMemcpyHostToDevice));
  ZKR_HIP_CHECK(hipMemcpy(add.p, addends_mont, n * sizeof(Affine<W>), hipMemcpyHostToDevice));
  if ((rc = add_each_launch<C>(pts.as<Affine<W>>(), pts.as<Affine<W>>(), add.as<Affine<W>>(), n, nullptr, n, ztmp.p, nullptr))) return rc;
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { set_error("adding the points failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  ZKR_HIP_CHECK(hipMemcpy(points_mont, pts.p, n * sizeof(Affine<W>), hipMemcpyDeviceToHost));
  return 0;
}

// The two point tables, into the room key_eval_rows made, on the key's device, under k->mu with no proof in flight.  0 with *why = null: both are in k->eval;
// 0 with a reason: the key keeps the coefficient form (nothing is left allocated); below zero: a kernel or a copy failed.
int derive_points(zkr_key *k, const Circuit &c, const unsigned char *base, const char **why) {
  const ArenaHeader &h = k->h;
  const uint32_t n = h.n, m = h.m;
  const int lt = k->layout.sort_src[T_C];  // the table whose sort C's accumulation reads: C' has its points, slot for slot
  const uint32_t np_c = h.npts[lt];
  ArenaHeader b;
  base_layout(h, b);
  const G1Affine *base_h = (const G1Affine *)(base + b.off_pts[T_H]), *base_c = (const G1Affine *)(base + b.off_pts[T_C]);
  EvalTables &ev = k->eval;
  *why = nullptr;
  auto give_up = [&](const char *reason) { (void)hipGetLastError(); key_eval_tables_free(k); *why = reason; return 0; };
  const char *const no_memory = "the device has no memory for the side tables";

  const size_t n_z = m > np_c ? m : np_c;
  DevBuf pw, tmp, tw, ztmp, sc;
  if (pw.alloc((size_t)m * sizeof(G1Affine)) || tmp.alloc((size_t)m * sizeof(G1Affine)) || tw.alloc(((size_t)m / 2 + 1) * sizeof(Fr)) ||
      ztmp.alloc(2 * n_z * sizeof(Fq)) || sc.alloc((size_t)m * sizeof(Fr)))
    return give_up(no_memory);
  G1Affine *P = pw.as<G1Affine>();
  const unsigned grid_m = (m + 255) / 256;
  int rc;
  // level 0 is in place: infinity in the wire form, then the window levels as the arena's own tables get them
  auto finish_table = [&](void *table, uint32_t np, const MsmPlan &pl) -> int {
    group_inf_wire_kernel<Fq><<<(np + 255) / 256, 256>>>((G1Affine *)table, np);
    ZKR_HIP_CHECK(hipGetLastError());
    return msm_precompute(k->device, false, table, np, pl);
  };

  // E': the key stores H bit-reversed (slot j = power bitrev(j)); power order, each power times ke g^(-i), the inverse transform
  {
    Fr two = Fr::zero(), mm = Fr::zero();
    two.v[0] = 2;
    mm.v[0] = m;
    const Fr half = inv(to_mont(two)), minv = inv(to_mont(mm)), ginv = inv(fr_root_of_unity(h.logm + 1));
    std::vector<Fr> e_sc(m);
    Fr cur = neg(mul(mul(half, Fr::r2()), mul(minv, minv)));  // ke, as eval_h_scalars has it
    for (uint32_t i = 0; i < m; i++) { e_sc[i] = from_mont(cur); cur = mul(cur, ginv); }
    ZKR_HIP_CHECK(hipMemcpy(sc.p, e_sc.data(), (size_t)m * sizeof(Fr), hipMemcpyHostToDevice));
    group_bitrev_kernel<Fq><<<grid_m, 256>>>(base_h, P, (int)h.logm);
    ZKR_HIP_CHECK(hipGetLastError());
    if ((rc = g1_scale_each(P, m, sc.as<Fr>(), 1, ztmp.p)) || (rc = g1_group_ntt(P, tmp.as<G1Affine>(), h.logm, true, tw.as<Fr>(), ztmp.p))) return rc;
    ZKR_HIP_CHECK(hipMemcpy(ev.e_pts, P, (size_t)m * sizeof(G1Affine), hipMemcpyDeviceToDevice));
    if ((rc = finish_table(ev.e_pts, m, k->plan[T_H]))) return rc;
    // 1/2 F: the same with one scalar for all
    const Fr half_std = from_mont(half);
    ZKR_HIP_CHECK(hipMemcpy(sc.p, &half_std, sizeof(Fr), hipMemcpyHostToDevice));
    group_bitrev_kernel<Fq><<<grid_m, 256>>>(base_h, P, (int)h.logm);
    ZKR_HIP_CHECK(hipGetLastError());
    if ((rc = g1_scale_each(P, m, sc.as<Fr>(), 0, ztmp.p)) || (rc = g1_group_ntt(P, tmp.as<G1Affine>(), h.logm, true, tw.as<Fr>(), ztmp.p))) return rc;
  }
  // C': per signal the combination of 1/2 F over its column of C (rows from nConstraints on are empty), added to the key's own C
  // point in the signal's slot of the layout
  {
    QapColumns cols;
    qap_columns(c, 2, cols);
    DevBuf comb;
    if ((rc = g1_combine_columns(n, cols, P, comb))) return rc;
    ZKR_HIP_CHECK(hipMemcpy(ev.c_pts, base_c, (size_t)np_c * sizeof(G1Affine), hipMemcpyDeviceToDevice));
    const uint32_t *rank = h.rank_identity[lt] ? nullptr : (const uint32_t *)(k->arena + h.off_rank[lt]);
    FaultCounter unplaced;
    if ((rc = unplaced.reset()) || (rc = add_each_launch<G1C>((G1Affine *)ev.c_pts, (const G1Affine *)ev.c_pts, comb.as<G1Affine>(), n, rank, np_c, ztmp.p, unplaced.dev())) ||
        (rc = unplaced.read()))
      return rc;
    if (unplaced.count) {
      static thread_local char msg[160];
      snprintf(msg, sizeof(msg), "%u signal(s) with a C' point have no slot among the points C's accumulation reads (first: signal %u)", unplaced.count, unplaced.first);
      return give_up(msg);
    }
    if ((rc = finish_table(ev.c_pts, np_c, k->plan[T_C]))) return rc;
  }
  return 0;
}

}  // namespace
}  // namespace zkr

using namespace zkr;

extern "C" {

int zkr_key_eval_tables(zkr_key *key, const void *r1cs_bin, size_t r1cs_len, unsigned flags, int *built) {
  if (!key || !r1cs_bin || !built) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (flags) { set_error("zkr_key_eval_tables: unknown flags %#x", flags); return ZKR_ERR_ARG; }
  *built = 0;
  Circuit c;
  if (int rc = parse_r1cs(r1cs_bin, r1cs_len, c)) return rc;  // before any device call: a malformed buffer is refused the same way everywhere
  if (zkr_device_count() < 1) { set_error("no HIP device; libzkr_hip has no CPU fallback"); return ZKR_ERR_NO_DEVICE; }
  const ArenaHeader &h = key->h;
  if (h.shard_parts != 1) { set_error("zkr_key_eval_tables: this key is shard %u of %u of a proving key; it takes a whole key", h.shard_part, h.shard_parts); return ZKR_ERR_ARG; }
  if (c.n != h.n || c.p != h.p || c.m != h.m) {
    set_error("zkr_key_eval_tables: the system has nVars=%u nPublic=%u domain=%u, the key %u, %u, %u", c.n, c.p, c.m, h.n, h.p, h.m);
    return ZKR_ERR_ARG;
  }
  void *base = nullptr;
  size_t base_len = 0;
  if (int rc = zkr_key_base_arena(key, &base, &base_len)) return rc;  // takes the key's lock itself
  ZKR_HIP_CHECK(hipSetDevice(key->device));
  std::lock_guard<std::mutex> lk(key->mu);  // no proof starts while the tables change
  if (int rc = refuse_in_flight(key, "zkr_key_eval_tables")) return rc;
  key_eval_tables_free(key);
  if (h_form_forced_coefficients()) { set_error("zkr_key_eval_tables: not built: ZKR_H_FORM=coefficients"); return 0; }
  if (!h.npts[T_C] || h.npts[T_H] != h.m) { set_error("zkr_key_eval_tables: not built: the key's H table dropped a point, or it has no C points"); return 0; }
  const char *why = nullptr;
  int rc = key_eval_rows(key, c);
  if (rc > 0) { rc = 0; why = "the device has no memory for the side tables"; }
  if (!rc && !why) rc = derive_points(key, c, (const unsigned char *)base, &why);
  if (rc || why) {
    (void)hipGetLastError();
    key_eval_tables_free(key);
    if (!rc) set_error("zkr_key_eval_tables: not built: %s", why);
    return rc;
  }
  key->eval.ready = true;
  *built = 1;
  return 0;
}

int zkr_key_eval_tables_drop(zkr_key *key) {
  if (!key) { set_error("null argument"); return ZKR_ERR_ARG; }
  ZKR_HIP_CHECK(hipSetDevice(key->device));
  std::lock_guard<std::mutex> lk(key->mu);
  if (int rc = refuse_in_flight(key, "zkr_key_eval_tables_drop")) return rc;
  return key_eval_tables_free(key);
}

int zkr_key_eval_tables_equal(const zkr_key *a, const zkr_key *b, int *same) {
  if (!a || !b || !same) { set_error("null argument"); return ZKR_ERR_ARG; }
  *same = 0;
  if (a->device != b->device) { set_error("zkr_key_eval_tables_equal: the keys live on devices %d and %d", a->device, b->device); return ZKR_ERR_ARG; }
  const EvalTables &x = a->eval, &y = b->eval;
  if (!x.ready || !y.ready) return 0;
  const int lt = a->layout.sort_src[T_C];
  // two shards: the same part of the same cut (their tables hold the shards' ranges, sized by the shards' own point counts)
  if (a->h.shard_parts != b->h.shard_parts || a->h.shard_part != b->h.shard_part || a->h.npts[T_H] != b->h.npts[T_H]) return 0;
  if (a->h.m != b->h.m || b->layout.sort_src[T_C] != lt || a->h.npts[lt] != b->h.npts[lt] || a->plan[T_C].K != b->plan[T_C].K || a->plan[T_H].K != b->plan[T_H].K ||
      x.nnz != y.nnz || x.n_wide != y.n_wide)
    return 0;
  ZKR_HIP_CHECK(hipSetDevice(a->device));
  bool eq = false;
  if (int rc = device_bytes_equal(a->device, x.c_pts, y.c_pts, (size_t)a->h.npts[lt] * a->plan[T_C].K * 64, &eq)) return rc;
  if (!eq) return 0;
  if (int rc = device_bytes_equal(a->device, x.e_pts, y.e_pts, (size_t)a->h.npts[T_H] * a->plan[T_H].K * 64, &eq)) return rc;
  if (!eq) return 0;
  // the C rows: small beside the tables, compared on the host
  const struct { const void *p, *q; size_t bytes; } rows[4] = {{x.c_rowptr, y.c_rowptr, ((size_t)a->h.m + 1) * 4}, {x.c_col, y.c_col, (size_t)x.nnz * 4},
                                                               {x.c_coef, y.c_coef, (size_t)x.nnz * 32}, {x.c_wide, y.c_wide, (size_t)x.n_wide * 4}};
  std::vector<uint8_t> u, v;
  for (const auto &r : rows) {
    if (!r.bytes) continue;
    u.resize(r.bytes); v.resize(r.bytes);
    ZKR_HIP_CHECK(hipMemcpy(u.data(), r.p, r.bytes, hipMemcpyDeviceToHost));
    ZKR_HIP_CHECK(hipMemcpy(v.data(), r.q, r.bytes, hipMemcpyDeviceToHost));
    if (memcmp(u.data(), v.data(), r.bytes) != 0) return 0;
  }
  *same = 1;
  return 0;
}

int zkr_points_add_each(void *points_mont, const void *addends_mont, size_t n, int g2, int device) {
  if (!points_mont || !addends_mont) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (n > 0xffffffffu) { set_error("zkr_points_add_each: at most 2^32 - 1 points"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  ZKR_HIP_CHECK(hipSetDevice(device));
  if (!n) return 0;
  return g2 ? add_each_hook<G2C>(points_mont, addends_mont, n) : add_each_hook<G1C>(points_mont, addends_mont, n);
}

}  // extern "C"
