// zkr_key_audit.hip -- the audit of a finished key by somebody who took no part in its ceremony: are this proving key and this
// verifying key the ones this circuit and this transcript give, with delta moved only by the recorded contributors?
//
// The setup (zkr_setup_r1cs_ptau, zkr_ptau.hip) takes the transcript's points to the Lagrange basis by NTTs over points and
// combines them per signal.  The audit stays on the SCALAR side, so an error in that derivation cannot agree with itself here: for
// random rho_s the polynomial sum_s rho_s A_s(x) has the values u[j] = sum_s polsA[s][j] rho_s on the domain -- the prover's own row
// product with rho in the witness's place -- and the coefficients a = iNTT_m(u), so that
//     sum_s rho_s A_s(tau) G = sum_i a_i tau^i G,
// an MSM over the transcript's monomial-basis points as they stand.  The same for B, for the circuit's C, and with alfa tau^i,
// beta tau^i for the combined query K[s] = beta A_s + alfa B_s + C_s (IC up to nPublic, C above).  No transform over points.
//
//   E1  sum_s rho_s A[s]   == sum_i a(rho)_i tauG1[i]
//   E2  sum_s rho_s B1[s]  == sum_i b(rho)_i tauG1[i]
//   E3  sum_s rho_s B2[s]  == sum_i b(rho)_i tauG2[i]
//   E4  sum_{s<=p} rho_s IC[s] == T(rho_pub)                    T(v) = sum_i a(v)_i betaTauG1[i] + b(v)_i alfaTauG1[i] + c(v)_i tauG1[i]
//   E5  e(sum_{s>p} rho_s C[s], delta2) == e(T(rho_priv), G2)
//   E6  e(sum_i sigma_i hExps[i], delta2) == e(sum_i sigma_i (tauG1[i+m] - tauG1[i]), G2)
// rho_s, sigma_i: 128 bits each from the OS CSPRNG (a wrong entry slips through with probability 2^-128); E5 and E6 share one
// pairing product, as step 5 of zkr_key_contribution_verify does.
//
// Everything heavy is a call the library already has: zkr_ptau_verify's steps (ptau_verify_keep leaves the verified transcript on
// the device, uploaded once), zkr_r1cs_matches_key, the prover's row kernels and its inverse transform with
// twiddle tables built for the call (a key's own are bytes of its file), the keys' MSM path over the
// key's tables (key_table_msm, key_table_msm_g2) and over the transcript's vectors (device_points_msm: one vector's window levels
// at a time), the pairings on the host.  New here: the kernel that makes the three masked scalar vectors from the 16-byte draws, and the row
// products of the system's C side.
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "kernels_ntt.hpp"  // spmv_kernel / spmv_wide_kernel, bitrev_copy_kernel
#include "hostops.hpp"
#include "pairing.hpp"
#include "record_util.hpp"
#include "zkr_internal.hpp"

namespace zkr {

// draws: n x 16 bytes.  out: three vectors of n scalars (32 B, standard form) end to end -- rho; rho on the signals 0..p and zero
// above (rho_pub); zero on 0..p and rho above (rho_priv).  Sixteen-byte loads and stores, a scalar = two of them.
static __global__ __launch_bounds__(256) void audit_scalars_kernel(const uint4 *draws, uint32_t n, uint32_t p, uint4 *out) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint4 d = draws[s], zero = make_uint4(0, 0, 0, 0);
  const uint32_t pub = s <= p ? 0xffffffffu : 0u, priv = ~pub;  // masks, word by word: a select between whole uint4 goes through the stack
  out[2 * (size_t)s] = d;
  out[2 * (size_t)s + 1] = zero;
  out[2 * ((size_t)n + s)] = make_uint4(d.x & pub, d.y & pub, d.z & pub, d.w & pub);
  out[2 * ((size_t)n + s) + 1] = zero;
  out[2 * (2 * (size_t)n + s)] = make_uint4(d.x & priv, d.y & priv, d.z & priv, d.w & priv);
  out[2 * (2 * (size_t)n + s) + 1] = zero;
}

// The system's C side times nvec vectors in the witness's place (blockIdx.y; vectors of n words end to end, standard form below r):
// out[j m + c] = row c times vector j below nConstraints, zero up to the domain's end -- C has nothing on the rows the setup appends
// to A.  Montgomery coefficient x standard word = standard word, as spmv_kernel, and the same split: one thread per row here, the
// rows of more than wide_terms terms left to audit_c_rows_wide_kernel.
static __global__ __launch_bounds__(256) void audit_c_rows_kernel(const uint32_t *row_ptr, const uint32_t *col, const Fr *coef, const Fr *v, uint32_t n, uint32_t nC, uint32_t m,
                                                                   uint32_t wide_terms, Fr *out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  v += (size_t)blockIdx.y * n;
  out += (size_t)blockIdx.y * m;
  Fr acc = Fr::zero();
  if (c < nC) {
    const uint32_t k0 = row_ptr[c], k1 = row_ptr[c + 1];
    if (k1 - k0 > wide_terms) return;
    for (uint32_t k = k0; k < k1; k++) acc = add(acc, mul(load_fr(coef + k), load_fr(v + col[k])));
  }
  store_fr(out + c, acc);
}
// wide[i] = the system's i-th constraint with ANY side of more than wide_terms terms (its list for zkr_r1cs_check): one wavefront
// each, four to a block; those whose C side is that wide have their terms strided over the lanes and summed by shuffles, the
// others were written by the kernel above.
static __global__ __launch_bounds__(256) void audit_c_rows_wide_kernel(const uint32_t *row_ptr, const uint32_t *col, const Fr *coef, const Fr *v, uint32_t n, uint32_t m,
                                                                        const uint32_t *wide, uint32_t n_wide, uint32_t wide_terms, Fr *out) {
  const uint32_t i = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
  if (i >= n_wide) return;  // uniform over the wavefront
  const uint32_t c = wide[i], k0 = row_ptr[c], k1 = row_ptr[c + 1];
  if (k1 - k0 <= wide_terms) return;
  v += (size_t)blockIdx.y * n;
  out += (size_t)blockIdx.y * m;
  Fr acc = Fr::zero();
  for (uint32_t k = k0 + lane; k < k1; k += 64) acc = add(acc, mul(load_fr(coef + k), load_fr(v + col[k])));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Fr y;
#pragma unroll
    for (int w = 0; w < 8; w++) y.v[w] = __shfl_xor(acc.v[w], o);
    acc = add(acc, y);
  }
  if (lane == 0) store_fr(out + c, acc);
}

namespace {

constexpr size_t REC_D1B = 0, REC_D1A = 64, REC_D2A = 128;  // the delta record's members (zkr_contribute.hip)
constexpr size_t VK_ALFA1 = 0, VK_BETA2 = 64, VK_GAMMA2 = 192, VK_DELTA2 = 320, VK_NIC = 448, VK_IC = 452;
const char *const TABLE_NAME[N_TABLES] = {"A", "B1", "B2", "C", "hExps"};

// null when the chain holds; else *bad = the record and `why` what failed
bool chain_valid(const uint8_t *records, size_t n, size_t *bad, char *why, size_t why_len) {
  uint8_t gen[64];
  store_g1_std(gen, g1_generator());
  for (size_t j = 0; j < n; j++) {
    const uint8_t *rec = records + j * ZKR_CONTRIBUTION_BYTES;
    *bad = j;
    int ok = 0;
    if (zkr_contribution_check(rec, &ok) || !ok) { snprintf(why, why_len, "record %zu: %s", j, zkr_last_error()); return false; }
    const uint8_t *want = j == 0 ? gen : rec - ZKR_CONTRIBUTION_BYTES + REC_D1A;
    if (memcmp(rec + REC_D1B, want, 64) != 0) {
      snprintf(why, why_len, j == 0 ? "record %zu: the chain does not start at the generator (delta1_before)" : "record %zu: the chain is broken (delta1_before is not the previous record's delta1_after)", j);
      return false;
    }
  }
  return true;
}

template <class F>
bool same_xyzz(const XYZZ<F> &a, const XYZZ<F> &b) {
  if (a.is_inf() || b.is_inf()) return a.is_inf() && b.is_inf();
  const Affine<F> x = to_affine(a), y = to_affine(b);
  return x.x == y.x && x.y == y.y;
}
G1XYZZ neg_xyzz(const G1XYZZ &a) {
  if (a.is_inf()) return a;
  const G1Affine p = to_affine(a);
  return to_xyzz(G1Affine{p.x, neg(p.y)});
}

}  // namespace
}  // namespace zkr

using namespace zkr;

extern "C" {

int zkr_contribution_chain_check(const uint8_t *records, size_t n_records, int *valid) {
  if (!valid || (n_records && !records)) { set_error("null argument"); return ZKR_ERR_ARG; }
  char why[320];
  size_t bad = 0;
  *valid = chain_valid(records, n_records, &bad, why, sizeof(why)) ? 1 : 0;
  if (!*valid) set_error("contribution chain check: %s", why);
  return 0;
}

int zkr_key_audit(const zkr_key *key, zkr_r1cs *cs, const void *ptau, size_t ptau_len, const uint8_t *ptau_records, size_t n_ptau_records, const uint8_t *delta_records,
                  size_t n_delta_records, const void *vk_bin, size_t vk_len, int *valid, uint64_t report[4]) {
  if (!ptau || !vk_bin || !valid || (n_ptau_records && !ptau_records) || (n_delta_records && !delta_records)) { set_error("null argument"); return ZKR_ERR_ARG; }
  *valid = 0;
  uint64_t rep_local[4];
  uint64_t *rep = report ? report : rep_local;
  rep[0] = rep[1] = 0;
  rep[2] = n_ptau_records;
  rep[3] = n_delta_records;
  // what can be refused from the bytes alone, before the key is looked at (a null handle is never read) and before any device call
  unsigned power = 0;
  if (const char *f = ptau_shape_fault(ptau, ptau_len, &power)) { set_error("zkr_key_audit: the transcript: %s", f); return ZKR_ERR_ARG; }
  const uint8_t *vk = (const uint8_t *)vk_bin;
  uint32_t n_ic = 0;
  if (vk_len >= VK_IC) memcpy(&n_ic, vk + VK_NIC, 4);
  if (vk_len < VK_IC || vk_len != VK_IC + 64ull * n_ic) { set_error("zkr_key_audit: verifying key length %zu does not match its IC count", vk_len); return ZKR_ERR_ARG; }
  if (!key || !cs) { set_error("null argument"); return ZKR_ERR_ARG; }
  const ArenaHeader &h = key->h;
  if (h.shard_parts > 1) { set_error("zkr_key_audit: this key is shard %u of %u of a proving key; it takes a whole key", h.shard_part, h.shard_parts); return ZKR_ERR_ARG; }
  R1csView sys;
  r1cs_view(cs, &sys);
  if (sys.device != key->device) { set_error("zkr_key_audit: the system is on device %d, the key on device %d", sys.device, key->device); return ZKR_ERR_ARG; }
  if (n_ic != h.p + 1) { set_error("zkr_key_audit: the verifying key has %u IC points, the key nPublic + 1 = %u", n_ic, h.p + 1); return ZKR_ERR_ARG; }
  const int device = key->device;
  const uint32_t n = h.n, p = h.p, m = h.m;
  const uint8_t *pt = (const uint8_t *)ptau;

  auto fail = [&](uint64_t step, uint64_t detail, const char *what) {
    rep[0] = step; rep[1] = detail;
    const std::string w(what);  // `what` may be zkr_last_error's own buffer
    set_error("key audit: step %llu failed: %s", (unsigned long long)step, w.c_str());
    return 0;
  };

  // 1. the transcript: zkr_ptau_verify's steps 2-6 with its records; what verified stays on the device
  PtauOnDevice tr;
  {
    int ok = 0;
    uint64_t prep[2] = {0, 0};
    if (int rc = ptau_verify_keep(ptau, ptau_len, ptau_records, n_ptau_records, device, &ok, prep, &tr)) return rc;
    if (!ok) return fail(1, 0, zkr_last_error());
  }
  // 2. the circuit: the domain fits the transcript, and the key's A and B sides are the system's
  {
    if ((uint64_t)m > (uint64_t)tr.M) {
      char msg[160];
      snprintf(msg, sizeof(msg), "the key's domain is %u; a transcript of power %u serves domains up to 2^%u", m, tr.power, tr.power);
      return fail(2, 0, msg);
    }
    int same = 0;
    if (int rc = zkr_r1cs_matches_key(cs, key, &same)) return rc;
    if (!same) return fail(2, 0, zkr_last_error());
  }
  // 3. the delta chain, and its end is this key's delta
  const G1Affine d1 = load_g1(h.delta1);
  const G2Affine d2 = load_g2(h.delta2);
  uint8_t d1_std[64], d2_std[128];
  {
    char why[320];
    size_t bad = 0;
    if (!chain_valid(delta_records, n_delta_records, &bad, why, sizeof(why))) return fail(3, bad, why);
    if (d1.is_inf() || d2.is_inf()) return fail(3, 0, "the key's delta is the point at infinity");
    store_g1_std(d1_std, d1);
    store_g2_std(d2_std, d2);
    uint8_t g1[64], g2[128];
    store_g1_std(g1, g1_generator());
    store_g2_std(g2, g2_generator());
    const uint8_t *last = n_delta_records ? delta_records + (n_delta_records - 1) * ZKR_CONTRIBUTION_BYTES : nullptr;
    if (memcmp(d1_std, last ? last + REC_D1A : g1, 64) != 0 || memcmp(d2_std, last ? last + REC_D2A : g2, 128) != 0)
      return fail(3, last ? n_delta_records - 1 : 0, last ? "the last record's delta1_after / delta2_after are not the key's delta" : "no delta records, but the key's delta is not the generators (delta = 1)");
  }
  // 4. the constants of both keys are the transcript's
  {
    uint8_t a1[64], b1[64], b2[128], g2[128];
    store_g1_std(a1, load_g1(h.alfa1));
    store_g1_std(b1, load_g1(h.beta1));
    store_g2_std(b2, load_g2(h.beta2));
    store_g2_std(g2, g2_generator());
    if (memcmp(a1, pt + tr.off_alfa1, 64) != 0) return fail(4, 0, "the key's alfa1 is not the transcript's alfaTauG1[0]");
    if (memcmp(b1, pt + tr.off_beta1, 64) != 0) return fail(4, 0, "the key's beta1 is not the transcript's betaTauG1[0]");
    if (memcmp(b2, pt + tr.off_beta2, 128) != 0) return fail(4, 0, "the key's beta2 is not the transcript's betaG2");
    if (memcmp(vk + VK_ALFA1, pt + tr.off_alfa1, 64) != 0) return fail(4, 0, "vk_alfa_1 is not the transcript's alfaTauG1[0]");
    if (memcmp(vk + VK_BETA2, pt + tr.off_beta2, 128) != 0) return fail(4, 0, "vk_beta_2 is not the transcript's betaG2");
    if (memcmp(vk + VK_GAMMA2, g2, 128) != 0) return fail(4, 0, "vk_gamma_2 is not the generator of G2 (gamma = 1)");
    if (memcmp(vk + VK_DELTA2, d2_std, 128) != 0) return fail(4, 0, "vk_delta_2 is not the key's delta2");
  }
  // 5. the window levels of all five tables are the multiples of their own base points, and the twiddle sections are the tables
  //    of the key's domain: each rebuilt and compared byte for byte, one table at a time (the peak is the largest table, and
  //    nothing stays on the key).  The sums below go through the key's MSM path, which reads those levels; the twiddles are what
  //    the key's prover would transform with -- the audit's own transforms never read them (fresh_scalar_intt).
  {
    bool same = false;
    if (int rc = key_twiddles_fresh_equal(key, &same)) return rc;
    if (!same) return fail(5, N_TABLES, "the twiddle tables are not the powers of the domain's root of unity");
    for (int t = 0; t < N_TABLES; t++) {
      if (!h.npts[t]) continue;
      const MsmPlan pl = msm_plan(rank_entries(h, t), h.npts[t], (int)h.win_c[t]);  // as key_build and arena_from_base plan it
      const size_t pb = t == T_B2 ? 128 : 64, bytes = (size_t)h.npts[t] * (size_t)pl.K * pb;
      if ((uint64_t)pl.K != (255 + (uint64_t)h.win_c[t] - 1) / h.win_c[t]) return fail(5, (uint64_t)t, "the table's window does not give the levels its section holds");
      DevBuf tbl;
      if (int rc = tbl.alloc(bytes)) return rc;
      ZKR_HIP_CHECK(hipSetDevice(device));
      ZKR_HIP_CHECK(hipMemcpy(tbl.p, key->arena + h.off_pts[t], (size_t)h.npts[t] * pb, hipMemcpyDeviceToDevice));  // level 0: the base points
      int rc;
      if ((rc = radix_convert(device, t == T_B2, tbl.p, h.npts[t], false)) || (rc = msm_precompute(device, t == T_B2, tbl.p, h.npts[t], pl)) ||
          (rc = device_bytes_equal(device, key->arena + h.off_pts[t], tbl.p, bytes, &same)))
        return rc;
      if (!same) {
        char msg[120];
        snprintf(msg, sizeof(msg), "the window levels of the %s table are not the multiples of its base points", TABLE_NAME[t]);
        return fail(5, (uint64_t)t, msg);
      }
    }
  }

  // ---- the scalar side: rho, rho_pub, rho_priv; their row products over the key's A and B and the system's C; the coefficients
  ZKR_HIP_CHECK(hipSetDevice(device));
  DevBuf d_rho, d_ev, d_co, d_sig, d_sig_h;
  int rc;
  {
    std::vector<uint8_t> draws((size_t)n * 16), sigma;
    DevBuf d_draws;
    if ((rc = os_random(draws.data(), draws.size())) || (rc = random_128(sigma, m))) return rc;  // rho: random_128's draws, expanded on the device
    if ((rc = d_draws.alloc(draws.size())) || (rc = d_rho.alloc((size_t)3 * n * 32)) || (rc = d_ev.alloc((size_t)9 * m * 32)) || (rc = d_co.alloc((size_t)9 * m * 32)) ||
        (rc = d_sig.alloc((size_t)m * 32)) || (rc = d_sig_h.alloc((size_t)m * 32)))
      return rc;
    ZKR_HIP_CHECK(hipMemcpy(d_draws.p, draws.data(), draws.size(), hipMemcpyHostToDevice));
    ZKR_HIP_CHECK(hipMemcpy(d_sig.p, sigma.data(), sigma.size(), hipMemcpyHostToDevice));
    audit_scalars_kernel<<<(n + 255) / 256, 256>>>(d_draws.as<uint4>(), n, p, d_rho.as<uint4>());
    // the H table pairs scalar position j with hExps[bitrev(j)] (the prover's h comes out bit-reversed): sigma in that order
    bitrev_copy_kernel<<<(m + 255) / 256, 256>>>(d_sig.as<Fr>(), d_sig_h.as<Fr>(), (int)h.logm);
    Fr *ev = d_ev.as<Fr>();
    const unsigned char *ar = key->arena;
    SpmvSide side[2];
    for (int i = 0; i < 2; i++)
      side[i] = SpmvSide{(const uint32_t *)(ar + h.off_rowptr[i]), (const uint32_t *)(ar + h.off_col[i]), (const Fr *)(ar + h.off_coef[i]), ev + (size_t)3 * i * m,
                         (const uint32_t *)(ar + h.off_wide[i]), h.n_wide[i]};
    spmv_kernel<<<dim3((m + 255) / 256, 3, 2), 256>>>(side[0], side[1], SpmvSide{}, d_rho.as<Fr>(), m, n, 0, m, nullptr);
    const uint32_t nw = h.n_wide[0] > h.n_wide[1] ? h.n_wide[0] : h.n_wide[1];
    if (nw) spmv_wide_kernel<<<dim3(nw, 3, 2), 64>>>(side[0], side[1], SpmvSide{}, d_rho.as<Fr>(), m, n, 0, m);
    // step 2 made the system's nVars, nPublic and domain the key's; its wide list holds constraints below nConstraints <= m
    audit_c_rows_kernel<<<dim3((m + 255) / 256, 3), 256>>>(sys.row_ptr[2], sys.col[2], sys.coef[2], d_rho.as<Fr>(), n, sys.nC, m, sys.wide_terms, ev + (size_t)6 * m);
    if (sys.n_wide)
      audit_c_rows_wide_kernel<<<dim3((sys.n_wide + 3) / 4, 3), 256>>>(sys.row_ptr[2], sys.col[2], sys.coef[2], d_rho.as<Fr>(), n, m, sys.wide, sys.n_wide, sys.wide_terms, ev + (size_t)6 * m);
    ZKR_HIP_CHECK(hipGetLastError());
    if ((rc = fresh_scalar_intt(device, h.logm, ev, d_co.as<Fr>(), 9))) return rc;
    const hipError_t e = hipDeviceSynchronize();  // `draws` goes with this scope
    if (e != hipSuccess) { set_error("key audit: the scalar side failed: %s", hipGetErrorString(e)); return ZKR_ERR_HIP; }
  }
  const Fr *rho = d_rho.as<Fr>(), *rho_priv = rho + (size_t)2 * n;
  enum { RHO = 0, PUB = 1, PRIV = 2 };
  auto co = [&](int side, int which) { return (const Fr *)(d_co.as<Fr>() + ((size_t)3 * side + which) * m); };

  // ---- the sums over the transcript's vectors, one vector's window levels at a time
  G1XYZZ s_tau[5], s_hi, s_alfa[2], s_beta[2];
  G2XYZZ s_tau2;
  {
    const Fr *sc_tau[5] = {co(0, RHO), co(1, RHO), co(2, PUB), co(2, PRIV), d_sig.as<Fr>()};
    const Fr *sc_hi[1] = {d_sig.as<Fr>()}, *sc_alfa[2] = {co(1, PUB), co(1, PRIV)}, *sc_beta[2] = {co(0, PUB), co(0, PRIV)}, *sc_tau2[1] = {co(1, RHO)};
    if ((rc = device_points_msm(device, false, tr.tau1, m, sc_tau, 5, s_tau)) || (rc = device_points_msm(device, false, tr.tau1 + m, m, sc_hi, 1, &s_hi)) ||
        (rc = device_points_msm(device, false, tr.alfa1, m, sc_alfa, 2, s_alfa)) || (rc = device_points_msm(device, false, tr.beta1, m, sc_beta, 2, s_beta)) ||
        (rc = device_points_msm(device, true, tr.tau2, m, sc_tau2, 1, &s_tau2)))
      return rc;
  }
  // 6. E1, E2, E3
  {
    G1XYZZ a_sum, b1_sum;
    G2XYZZ b2_sum;
    if ((rc = key_table_msm(key, T_A, rho, &a_sum)) || (rc = key_table_msm(key, T_B1, rho, &b1_sum)) || (rc = key_table_msm_g2(key, rho, &b2_sum))) return rc;
    if (!same_xyzz(a_sum, s_tau[0])) return fail(6, T_A, "the A points are not sum_j polsA[s][j] L_j(tau) G1 of this circuit and transcript");
    if (!same_xyzz(b1_sum, s_tau[1])) return fail(6, T_B1, "the B1 points are not sum_j polsB[s][j] L_j(tau) G1 of this circuit and transcript");
    if (!same_xyzz(b2_sum, s_tau2)) return fail(6, T_B2, "the B2 points are not sum_j polsB[s][j] L_j(tau) G2 of this circuit and transcript");
  }
  // 7. E4: the verifying key's IC
  {
    std::vector<uint8_t> ic_mont((size_t)n_ic * 64), sc((size_t)n_ic * 32);
    for (uint32_t s = 0; s < n_ic; s++) {
      G1Affine q;
      if (!read_g1_std(vk + VK_IC + 64 * (size_t)s, q)) {
        char msg[96];
        snprintf(msg, sizeof(msg), "IC[%u] is at infinity, out of range or off the curve", s);
        return fail(7, 0, msg);
      }
      store_g1_mont(&ic_mont[64 * (size_t)s], q);
    }
    ZKR_HIP_CHECK(hipMemcpy(sc.data(), rho, sc.size(), hipMemcpyDeviceToHost));
    uint8_t o[64];
    int is_inf = 0;
    if ((rc = zkr_msm_g1(ic_mont.data(), sc.data(), n_ic, o, &is_inf, device))) return rc;
    G1XYZZ ic_sum = G1XYZZ::inf();
    if (!is_inf) ic_sum = to_xyzz(G1Affine{to_mont(load_fp<FqParams>(o)), to_mont(load_fp<FqParams>(o + 32))});
    const G1XYZZ want = add_full(add_full(s_beta[0], s_alfa[0]), s_tau[2]);
    if (!same_xyzz(ic_sum, want)) return fail(7, 0, "the verifying key's IC points are not beta A_s + alfa B_s + C_s of this circuit and transcript");
  }
  // 8. E5 and E6 in one pairing product
  {
    G1XYZZ c_sum, h_sum;
    if ((rc = key_table_msm(key, T_C, rho_priv, &c_sum)) || (rc = key_table_msm(key, T_H, d_sig_h.as<Fr>(), &h_sum))) return rc;
    const G1XYZZ lhs = add_full(c_sum, h_sum);
    const G1XYZZ rhs = add_full(add_full(add_full(s_beta[1], s_alfa[1]), s_tau[3]), add_full(s_hi, neg_xyzz(s_tau[4])));
    const char *what = "the C or hExps points are not (beta A_s + alfa B_s + C_s) / delta, tau^i Z(tau) / delta of this circuit, transcript and delta";
    if (lhs.is_inf() != rhs.is_inf()) return fail(8, 0, what);
    if (!lhs.is_inf() && !pairings_equal(to_affine(lhs), d2, to_affine(rhs), g2_generator())) return fail(8, 0, what);
  }
  *valid = 1;
  return 0;
}

}  // extern "C"
