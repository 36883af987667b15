// zkr_setup.hip -- Groth16 setup for an arbitrary R1CS: restates `snarkjs setup --protocol groth`
// (prover/package.json:34,37; SURVEY App. B "Setup").  Host logic here; the key's group elements are computed on the GPU by the
// fixed-base kernel (kernels_msm.hpp), so no multi-GB websnark binary ever exists on the host unless a caller asks for one.  The
// forms the circuit's QAP takes on the way -- by row as a key holds it, by signal -- are qap_forms.hpp's.
#include <stdlib.h>
#include <string.h>
#include "eval_h.hpp"
#include "verify_key.hpp"
#include "websnark_writer.hpp"
#include "zkr_setup.hpp"

namespace zkr {

static void setup_scalars(const Circuit &c, const Toxic &tx, SetupScalars &sc, bool secret) {
  uint32_t m = c.m, n = c.n, p = c.p;
  const unsigned logm = domain_log2(m);
  // L_c(t) = (t^m - 1) w^c / (m (t - w^c)) with one batch inversion
  Fr w = fr_root_of_unity(logm);
  std::vector<Fr> wc(m), den(m), pref(m);
  Fr cur = Fr::one();
  for (uint32_t i = 0; i < m; i++) { wc[i] = cur; den[i] = sub(tx.t, cur); cur = mul(cur, w); }
  Fr run = Fr::one();
  for (uint32_t i = 0; i < m; i++) { pref[i] = run; run = mul(run, den[i]); }
  Fr invall = inv(run);
  Fr tm = tx.t;
  for (unsigned i = 0; i < logm; i++) tm = sqr(tm);
  Fr z = sub(tm, Fr::one());
  Fr zm = mul(z, inv(fr_u64(m)));
  std::vector<Fr> L(m);
  for (uint32_t i = m; i-- > 0;) {
    Fr di = mul(invall, pref[i]);
    invall = mul(invall, den[i]);
    L[i] = mul(mul(zm, wc[i]), di);
  }
  std::vector<Fr> *at_t[3] = {&sc.a, &sc.b, &sc.c};
  for (int s = 0; s < 3; s++) {
    const QapRows &q = c.side[s];
    std::vector<Fr> &v = *at_t[s];
    v.assign(n, Fr::zero());
    for (uint32_t r = 0; r < c.nC; r++)
      for (uint32_t k = q.rowptr[r]; k < q.rowptr[r + 1]; k++) v[q.sig[k]] = add(v[q.sig[k]], mul(q.coef[k], L[r]));
  }
  for (uint32_t i = 0; i <= p; i++) sc.a[i] = add(sc.a[i], L[c.nC + i]);  // input-consistency rows polsA[i][nC+i] = 1
  Fr ginv = inv(tx.gamma), dinv = inv(tx.delta);
  sc.ic.resize(p + 1);
  sc.cpriv.resize(n - p - 1);
  for (uint32_t s = 0; s < n; s++) {
    Fr k = add(add(mul(tx.beta, sc.a[s]), mul(tx.alfa, sc.b[s])), sc.c[s]);
    if (s <= p) sc.ic[s] = mul(k, ginv); else sc.cpriv[s - p - 1] = mul(k, dinv);
  }
  sc.hx.resize(m);
  Fr ti = mul(z, dinv);
  for (uint32_t i = 0; i < m; i++) { sc.hx[i] = ti; ti = mul(ti, tx.t); }
  if (secret) { wipe_vector(den); wipe_vector(pref); wipe_vector(L); }  // t - w^c, their products, L_c(t): each reveals t
}

int setup_from_circuit(int device, Generated &g) {
  if (int rc = need_device(device)) return rc;
  setup_scalars(g.circ, g.tox, g.sc, g.secret);
  struct Staging {  // standard-form copies of the scalars on their way to the device: wiped with the rest
    std::vector<uint8_t> v;
    bool secret;
    ~Staging() { if (secret) wipe_vector(v); }
  } stage{{}, g.secret};
  std::vector<uint8_t> &bytes = stage.v;
  int rc;
  const std::vector<Fr> *src[N_TABLES] = {&g.sc.a, &g.sc.b, &g.sc.b, &g.sc.cpriv, &g.sc.hx};
  for (int t = 0; t < N_TABLES; t++) {
    if (g.secret) wipe_vector(bytes);
    to_std_bytes(*src[t], bytes);
    if ((rc = fixed_base_points(device, t == T_B2, bytes.data(), src[t]->size(), g.d_tbl[t], g.secret))) return rc;
  }
  // vk_alfa_1, vk_beta_1, vk_delta_1 | vk_beta_2, vk_delta_2  (header layout binarify.ts:163-167)
  std::vector<Fr> g1s = {g.tox.alfa, g.tox.beta, g.tox.delta}, g2s = {g.tox.beta, g.tox.delta, g.tox.gamma};
  DevBuf d;
  if (g.secret) wipe_vector(bytes);
  to_std_bytes(g1s, bytes);
  if ((rc = fixed_base_points(device, false, bytes.data(), 3, d, g.secret))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(g.consts, d, 192, hipMemcpyDeviceToHost));
  to_std_bytes(g2s, bytes);
  if ((rc = fixed_base_points(device, true, bytes.data(), 3, d, g.secret))) return rc;
  if (g.secret) { wipe_vector(g1s); wipe_vector(g2s); }
  uint8_t g2pts[384];
  ZKR_HIP_CHECK(hipMemcpy(g2pts, d, 384, hipMemcpyDeviceToHost));
  memcpy(g.consts + 192, g2pts, 256);
  G2Affine gm = load_g2(g2pts + 256);
  g.gamma2_std.resize(128);
  store_g2_std(g.gamma2_std.data(), gm);
  // IC points for the checker
  if (g.secret) wipe_vector(bytes);
  to_std_bytes(g.sc.ic, bytes);
  if ((rc = fixed_base_points(device, false, bytes.data(), g.sc.ic.size(), d, g.secret))) return rc;
  std::vector<uint8_t> icm(g.sc.ic.size() * 64);
  ZKR_HIP_CHECK(hipMemcpy(icm.data(), d, icm.size(), hipMemcpyDeviceToHost));
  g.ic_std.resize(icm.size());
  for (size_t i = 0; i < g.sc.ic.size(); i++) store_g1_std(&g.ic_std[i * 64], load_g1(&icm[i * 64]));
  return 0;
}

// Which points of the tables a key keeps: a signal whose polynomial vanishes at t has the point at infinity and is dropped.
struct KeptPoints {
  std::vector<uint8_t> a, b, c, h;  // per signal (A; B1 and B2), per private signal s - nPublic - 1 (C), per power i (H)
};
// A and B as the key holds them, the kept points of every table, then the arena.
// d_tbl: device tables; the C point of private signal s is entry s - nPublic - 1 + c_src_base of d_tbl[T_C].
static int build_key_from_tables(const Circuit &c, const KeptPoints &keep, const DevBuf d_tbl[N_TABLES], uint32_t c_src_base, const uint8_t *consts448, int device,
                                 zkr_key **key_out) {
  const uint32_t n = c.n, p = c.p, m = c.m;
  KeySource ks;
  ks.n = n; ks.p = p; ks.m = m;
  ks.consts448 = consts448;
  for (int s = 0; s < 2; s++) key_rows(c, s, false, ks.side[s]);
  for (int t = 0; t < N_TABLES; t++) { ks.tbl[t].src = d_tbl[t]; ks.tbl[t].on_device = true; }
  auto kept = [&](int t, uint32_t src, uint32_t scalar) { ks.tbl[t].srcidx.push_back(src); ks.tbl[t].sidx.push_back(scalar); };
  for (uint32_t s = 0; s < n; s++) {
    if (keep.a[s]) kept(T_A, s, s);
    if (keep.b[s]) { kept(T_B1, s, s); kept(T_B2, s, s); }
  }
  for (uint32_t i = 0; i < n - p - 1; i++)
    if (keep.c[i]) kept(T_C, i + c_src_base, i + p + 1);
  const unsigned logm = domain_log2(m);
  for (uint32_t j = 0; j < m; j++) {
    const uint32_t i = bitrev32(j, logm);
    if (keep.h[i]) kept(T_H, i, j);
  }
  return key_build(device, ks, key_out);
}
int build_key_from_generated(const Generated &g, int device, zkr_key **key_out) {
  KeptPoints keep;
  auto nonzero = [](const std::vector<Fr> &v, std::vector<uint8_t> &k) {
    k.resize(v.size());
    for (size_t i = 0; i < v.size(); i++) k[i] = !v[i].is_zero();
  };
  nonzero(g.sc.a, keep.a); nonzero(g.sc.b, keep.b); nonzero(g.sc.cpriv, keep.c); nonzero(g.sc.hx, keep.h);
  return build_key_from_tables(g.circ, keep, g.d_tbl, 0, g.consts, device, key_out);
}

// The side tables of H in evaluation form (zkr_internal.hpp EvalTables; the algebra: eval_h.hpp) for a key this setup has just
// built: the scalars of C' and E' from the setup's own, their points by the fixed-base kernel, their window levels with the plans
// of C and H, C by QAP row for the prover's third row sum, and a counter per proof slot.  Returns 0 with the key unchanged -- it
// proves through the coefficient form -- when an allocation fails (refuse: the test hook that says so), when ZKR_H_FORM=coefficients
// asks for it, or when the tables would not fit the layout the key's proofs run on: the H table dropped a point, or a signal with a
// C' point has no place among the points of C (of A's sort, when the two share one).  Below zero only for a failed kernel.
int key_build_eval_tables(zkr_key *k, const Generated &g, bool refuse) {
  const ArenaHeader &h = k->h;
  const Circuit &c = g.circ;
  const uint32_t n = h.n, m = h.m, p = h.p;
  if (h_form_forced_coefficients()) return 0;
  if (refuse || h.shard_parts != 1 || !h.npts[T_C] || h.npts[T_H] != m) return 0;
  ZKR_HIP_CHECK(hipSetDevice(k->device));
  struct Secret {  // scalars that reveal t or delta go the way the setup's own do
    EvalHScalars es;
    std::vector<Fr> c_sc;
    std::vector<uint8_t> bytes;
    bool wipe;
    ~Secret() { if (wipe) { wipe_vector(es.f); wipe_vector(es.e); wipe_vector(es.cfold); wipe_vector(es.eprime); wipe_vector(c_sc); wipe_vector(bytes); } }
  } sec{{}, {}, {}, g.secret};
  const QapRows &qc = c.side[2];
  eval_h_scalars(g.sc.hx.data(), h.logm, qc.rowptr.data(), qc.sig.data(), qc.coef.data(), c.nC, n, p, g.sc.cpriv.data(), sec.es);
  // C' over the points of the table whose sort C's accumulation reads
  const int lt = k->layout.sort_src[T_C];
  const uint32_t np_c = h.npts[lt];
  std::vector<uint32_t> rank(n);
  if (h.rank_identity[lt]) for (uint32_t s = 0; s < n; s++) rank[s] = s;
  else ZKR_HIP_CHECK(hipMemcpy(rank.data(), k->arena + h.off_rank[lt], (size_t)n * 4, hipMemcpyDeviceToHost));
  sec.c_sc.assign(np_c, Fr::zero());
  for (uint32_t s = 0; s < n; s++) {
    if (sec.es.cfold[s].is_zero()) continue;
    if (rank[s] >= np_c) return 0;  // no point for this signal in the layout (0xffffffff: dropped)
    sec.c_sc[rank[s]] = sec.es.cfold[s];
  }
  EvalTables &ev = k->eval;
  auto give_up = [&](bool hip_failed) { if (hip_failed) (void)hipGetLastError(); key_eval_tables_free(k); return 0; };
  // level 0 from the scalars, then the window levels in place (msm_precompute)
  auto table = [&](const std::vector<Fr> &scalars, const MsmPlan &pl, void *out) -> int {
    const size_t np = scalars.size();
    to_std_bytes(scalars, sec.bytes);
    DevBuf lvl0;
    if (int rc = fixed_base_points(k->device, false, sec.bytes.data(), np, lvl0, g.secret)) return rc;
    hipError_t e = hipMemcpy(out, lvl0, np * 64, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { set_error("copy of a side table's base points failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
    return msm_precompute(k->device, false, out, (uint32_t)np, pl);
  };
  int rc;
  if ((rc = key_eval_rows(k, c)) > 0) return give_up(true);
  if (!rc) rc = table(sec.c_sc, k->plan[T_C], ev.c_pts);
  if (!rc) rc = table(sec.es.eprime, k->plan[T_H], ev.e_pts);
  if (rc) { give_up(false); return rc; }
  ev.ready = true;
  return 0;
}

// Room for a whole key's side tables (eval_tables_alloc; whoever fills the points: above, zkr_eval_tables.hip) and what they need
// beside their points: C by row over the whole domain (rows from nConstraints on are empty), STANDARD-form coefficients -- with the
// standard-form witness the row sums come out as c_j / R, which is what one product of a_j and b_j leaves (kernels_ntt.hpp
// eval_unsatisfied_kernel).  Above zero: an allocation failed (the caller gives the tables up); below: a failed copy.
int key_eval_rows(zkr_key *k, const Circuit &c) {
  EvalTables &ev = k->eval;
  KeyRows rows;
  key_rows(c, 2, true, rows);
  const std::vector<uint32_t> wide = wide_rows(rows.rowptr.data(), c.m);
  if (!eval_tables_alloc(k, k->h.npts[k->layout.sort_src[T_C]], k->h.m, (uint32_t)rows.col.size(), (uint32_t)wide.size())) return 1;
  hipError_t e = hipMemcpy(ev.c_rowptr, rows.rowptr.data(), rows.rowptr.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && !rows.col.empty()) e = hipMemcpy(ev.c_col, rows.col.data(), rows.col.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess && !rows.coef.empty()) e = hipMemcpy(ev.c_coef, rows.coef.data(), rows.coef.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess && !wide.empty()) e = hipMemcpy(ev.c_wide, wide.data(), wide.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { set_error("upload of the C rows failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  return 0;
}

int vk_to_malloc(const Generated &g, void **vk_out, size_t *vk_len) {
  std::vector<uint8_t> vk;
  write_vk(vk, g.consts, g.consts + 192, g.gamma2_std.data(), g.consts + 320, g.ic_std.data(), g.ic_std.size() / 64);
  return give_bytes(vk, vk_out, vk_len);
}

// binarify.ts:143-206 through the writer the export uses (websnark_writer.hpp): plan, header and pols sections from A and B as
// the key holds them, then the five device tables as they are
int render_websnark(const Generated &g, void **pk_out, size_t *pk_len) {
  const Circuit &c = g.circ;
  WebsnarkPlan pl;
  if (int rc = websnark_plan(c.n, c.p, c.m, c.side[0].sig.size() + c.p + 1, c.side[1].sig.size(), pl)) return rc;
  KeyRows side[2];
  for (int s = 0; s < 2; s++) key_rows(c, s, false, side[s]);
  uint8_t *o = (uint8_t *)malloc(pl.len);
  if (!o) { set_error("out of memory"); return ZKR_ERR_ARG; }
  const uint32_t *rp[2] = {side[0].rowptr.data(), side[1].rowptr.data()}, *cl[2] = {side[0].col.data(), side[1].col.data()};
  const uint8_t *cf[2] = {side[0].coef.data(), side[1].coef.data()};
  if (int rc = websnark_write_front(o, pl, c.n, c.p, c.m, g.consts, rp, cl, cf)) { free(o); return rc; }
  for (int t = 0; t < N_TABLES; t++) {
    const size_t bytes = pl.count[t] * WEBSNARK_POINT_BYTES[t];
    if (bytes && hipMemcpy(o + pl.ptr[2 + t], g.d_tbl[t], bytes, hipMemcpyDeviceToHost) != hipSuccess) { free(o); set_error("download of key table %d failed", t); return ZKR_ERR_HIP; }
  }
  *pk_out = o;
  *pk_len = pl.len;
  return 0;
}

}  // namespace zkr

using namespace zkr;

extern "C" {

static int draw_fr(Fr &out) {
  for (;;) {
    uint8_t b[32];
    if (int rc = os_random(b, 32)) return rc;
    b[31] &= 0x3f;
    if (read_fr_std(b, out) && !out.is_zero()) return 0;
  }
}

// r1cs_bin -> g.circ; toxic waste injected or drawn; QAP at t and every group element on the GPU
static int setup_parse_and_run(const void *r1cs_bin, size_t r1cs_len, const uint8_t *toxic160, int device, Generated &g) {
  if (int rc = parse_r1cs(r1cs_bin, r1cs_len, g.circ)) return rc;
  Fr *tox[5] = {&g.tox.t, &g.tox.alfa, &g.tox.beta, &g.tox.gamma, &g.tox.delta};
  if (toxic160) {
    for (int i = 0; i < 5; i++) {
      Fr v;
      if (!read_fr_std(toxic160 + 32 * i, v) || v.is_zero()) { set_error("toxic scalar %d is zero or >= r", i); return ZKR_ERR_ARG; }
      *tox[i] = to_mont(v);
    }
  } else {  // fresh toxic waste from the OS CSPRNG; it never leaves this call (Generated::~Generated wipes it and
            // everything derived from it, host and device copies)
    g.secret = true;
    for (int i = 0; i < 5; i++) {
      Fr v;
      if (int rc = draw_fr(v)) return rc;
      *tox[i] = to_mont(v);
    }
  }
  return setup_from_circuit(device, g);
}

// the caller gets both or neither
static int key_and_vk(const Generated &g, zkr_key **key_out, void **vk_out, size_t *vk_len) {
  int rc = vk_to_malloc(g, vk_out, vk_len);
  if (rc) { zkr_key_free(*key_out); *key_out = nullptr; }
  return rc;
}

int zkr_setup_r1cs_opts(const void *r1cs_bin, size_t r1cs_len, const uint8_t *toxic160, int device, unsigned flags, zkr_key **key_out, void **vk_out, size_t *vk_len) {
  if (!r1cs_bin || !key_out || !vk_out || !vk_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  Generated g;
  int rc = setup_parse_and_run(r1cs_bin, r1cs_len, toxic160, device, g);
  if (!rc) rc = build_key_from_generated(g, device, key_out);
  if (rc) return rc;
  if ((rc = key_build_eval_tables(*key_out, g, (flags & ZKR_SETUP_NO_SIDE_TABLES) != 0))) { zkr_key_free(*key_out); *key_out = nullptr; return rc; }
  return key_and_vk(g, key_out, vk_out, vk_len);
}
int zkr_setup_r1cs(const void *r1cs_bin, size_t r1cs_len, const uint8_t *toxic160, int device, zkr_key **key_out, void **vk_out, size_t *vk_len) {
  return zkr_setup_r1cs_opts(r1cs_bin, r1cs_len, toxic160, device, 0, key_out, vk_out, vk_len);
}

// The same key from a powers-of-tau transcript instead of toxic scalars (zkr_ptau.hip): nobody knows t, alfa, beta; delta = gamma = 1
int zkr_setup_r1cs_ptau(const void *r1cs_bin, size_t r1cs_len, const void *ptau, size_t ptau_len, int device, zkr_key **key_out, void **vk_out, size_t *vk_len) {
  if (!r1cs_bin || !ptau || !key_out || !vk_out || !vk_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  Generated g;
  Circuit &c = g.circ;
  int rc = parse_r1cs(r1cs_bin, r1cs_len, c);
  if (rc) return rc;
  const uint32_t n = c.n, p = c.p, m = c.m;
  QapColumns cols[3];
  for (int k = 0; k < 3; k++) qap_columns(c, k, cols[k]);
  if ((rc = ptau_key_tables(ptau, ptau_len, device, m, n, cols, g.d_tbl, g.consts))) return rc;
  // a table entry is dropped exactly when its point is infinity; the IC points for the verifying key
  KeptPoints keep;
  std::vector<uint8_t> host;
  auto finite = [&](int t, size_t count, size_t first, std::vector<uint8_t> &k) -> int {
    host.resize(count * 64);
    if (count) ZKR_HIP_CHECK(hipMemcpy(host.data(), (const uint8_t *)g.d_tbl[t] + first * 64, host.size(), hipMemcpyDeviceToHost));
    k.resize(count);
    for (size_t i = 0; i < count; i++) k[i] = !load_g1(&host[i * 64]).is_inf();
    return 0;
  };
  if ((rc = finite(T_H, m, 0, keep.h)) || (rc = finite(T_A, n, 0, keep.a)) || (rc = finite(T_B1, n, 0, keep.b)) || (rc = finite(T_C, n - p - 1, p + 1, keep.c))) return rc;
  host.resize((size_t)(p + 1) * 64);
  ZKR_HIP_CHECK(hipMemcpy(host.data(), g.d_tbl[T_C], host.size(), hipMemcpyDeviceToHost));
  g.ic_std.assign(host.size(), 0);
  for (uint32_t i = 0; i <= p; i++) {
    const G1Affine ic = load_g1(&host[(size_t)i * 64]);
    if (!ic.is_inf()) store_g1_std(&g.ic_std[(size_t)i * 64], ic);
  }
  g.gamma2_std.resize(128);
  store_g2_std(g.gamma2_std.data(), g2_generator());
  if ((rc = build_key_from_tables(c, keep, g.d_tbl, p + 1, g.consts, device, key_out))) return rc;
  return key_and_vk(g, key_out, vk_out, vk_len);
}

int zkr_setup_r1cs_websnark(const void *r1cs_bin, size_t r1cs_len, const uint8_t *toxic160, int device, void **pk_out, size_t *pk_len, void **vk_out, size_t *vk_len) {
  if (!r1cs_bin || !pk_out || !pk_len || !vk_out || !vk_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  Generated g;
  int rc = setup_parse_and_run(r1cs_bin, r1cs_len, toxic160, device, g);
  if (!rc) rc = render_websnark(g, pk_out, pk_len);
  if (rc) return rc;
  if ((rc = vk_to_malloc(g, vk_out, vk_len))) { free(*pk_out); *pk_out = nullptr; }
  return rc;
}

}  // extern "C"
