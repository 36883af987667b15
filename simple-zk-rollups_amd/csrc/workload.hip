// workload.hip -- seeded synthetic rollup-shaped R1CS and witness, and the zkr_synth_* entry points
// that run the Groth16 setup of zkr_setup.hip on it.
//
// The reference has no checked-in key or circuit artefact (prover/.gitignore:109), so benchmark inputs must be generated: a
// circuit drawn by the same SplitMix64 stream as oracle/groth16.py's synth_circuit -- tests/test_workload.py checks the two
// generators byte-for-byte at small sizes.
#include <stdlib.h>
#include <string.h>
#include <map>
#include "verify_key.hpp"
#include "zkr_setup.hpp"

namespace zkr {

struct SplitMix64 {
  uint64_t s;
  explicit SplitMix64(uint64_t seed) : s(seed) {}
  uint64_t u64() {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  Fr fr_std() {  // uniform in [0, r) by rejection, standard form
    for (;;) {
      uint64_t a = u64(), b = u64(), c = u64(), d = u64() & ((1ull << 62) - 1);
      Fr v;
      v.v[0] = (uint32_t)a; v.v[1] = (uint32_t)(a >> 32); v.v[2] = (uint32_t)b; v.v[3] = (uint32_t)(b >> 32);
      v.v[4] = (uint32_t)c; v.v[5] = (uint32_t)(c >> 32); v.v[6] = (uint32_t)d; v.v[7] = (uint32_t)(d >> 32);
      if (words_below(v.v, FrParams::P)) return v;
    }
  }
  Fr fr() { return to_mont(fr_std()); }
};

static Fr dot(const QapRows &q, size_t b, const std::vector<Fr> &w) {  // the terms from b on
  Fr acc = Fr::zero();
  for (size_t i = b; i < q.sig.size(); i++) acc = add(acc, mul(q.coef[i], w[q.sig[i]]));
  return acc;
}

// circuit shape of the zkr_synth_* entry points: 0 = rollup-shaped (default), 1 = dense random (BASELINE config 5)
static thread_local unsigned g_shape = 0;  // per calling thread (zkr_synth_set_shape): the library stays re-entrant

// draw-for-draw mirror of oracle/groth16.py:synth_circuit
static void synth_circuit(Circuit &c, uint32_t m, uint32_t p, uint64_t seed, uint64_t witness_seed) {
  SplitMix64 rng(seed);
  SplitMix64 rv(witness_seed ^ 0x77697473ull);  // free witness values: own stream, so one key serves many witnesses
  c.m = m; c.p = p; c.nC = m - p - 1;
  c.w.reserve(m + 8);
  c.w.push_back(Fr::one());
  for (uint32_t i = 0; i < p; i++) c.w.push_back(rv.fr());
  const Fr one = Fr::one(), minus1 = neg(Fr::one());
  QapRows &qa = c.side[0], &qb = c.side[1], &qc = c.side[2];
  auto term = [](QapRows &q, uint32_t sig, const Fr &coef) { q.sig.push_back(sig); q.coef.push_back(coef); };
  auto terms = [&](QapRows &q, const std::map<uint32_t, Fr> &by_signal) { for (auto &kv : by_signal) term(q, kv.first, kv.second); };
  auto end_row = [&]() { for (QapRows &q : c.side) q.rowptr.push_back((uint32_t)q.sig.size()); };
  end_row();
  for (uint32_t row = 0; row < c.nC; row++) {
    uint32_t n = (uint32_t)c.w.size();
    if (g_shape == 1) {  // (4 random signals, random coefficients) x (4 more) = new signal
      std::map<uint32_t, Fr> AB[2];
      for (auto &d : AB)
        for (int k = 0; k < 4; k++) {
          uint32_t j = (uint32_t)(rng.u64() % n);
          Fr cf = rng.fr();
          auto it = d.find(j);
          if (it == d.end()) d[j] = cf; else it->second = add(it->second, cf);
        }
      size_t ba = qa.sig.size(), bb = qb.sig.size();
      terms(qa, AB[0]);
      terms(qb, AB[1]);
      c.w.push_back(mul(dot(qa, ba, c.w), dot(qb, bb, c.w)));
      term(qc, n, one);
      end_row();
      continue;
    }
    uint64_t kind = rng.u64() % 100;
    if (row % 2048 == 1000) {
      std::map<uint32_t, Fr> A;
      Fr pw = one;
      for (int k = 0; k < 64; k++) {
        uint32_t j = (uint32_t)(rng.u64() % n);
        auto it = A.find(j);
        if (it == A.end()) A[j] = pw; else it->second = add(it->second, pw);
        pw = dbl(pw);
      }
      size_t b = qa.sig.size();
      terms(qa, A);
      c.w.push_back(dot(qa, b, c.w));
      term(qb, 0, one);
      term(qc, n, one);
    } else if (kind < 3) {
      uint64_t bit = rv.u64() & 1;
      c.w.push_back(bit ? one : Fr::zero());
      term(qa, n, one);
      term(qb, 0, minus1);
      term(qb, n, one);
    } else if (kind < 5) {
      c.w.push_back(fr_u64(rv.u64()));
      term(qa, n, one);
      term(qb, 0, one);
      term(qc, n, one);
    } else {
      uint32_t i = n - 1;
      uint64_t sel = rng.u64();
      uint32_t j = (uint32_t)(rng.u64() % n);
      uint32_t kk = 0;
      if (n > 1) { uint32_t lim = n - 1 < 16 ? n - 1 : 16; kk = n - 1 - (uint32_t)(rng.u64() % lim); }
      std::map<uint32_t, Fr> A, B;
      A[i] = one;
      if ((sel & 1) && j != i) A[j] = rng.fr();
      if (((sel >> 1) & 3) == 0 && !A.count(0)) A[0] = rng.fr();
      B[kk] = one;
      if (((sel >> 3) & 1) && kk != 0) B[0] = rng.fr();
      size_t ba = qa.sig.size(), bb = qb.sig.size();
      terms(qa, A);
      terms(qb, B);
      Fr val = mul(dot(qa, ba, c.w), dot(qb, bb, c.w));
      if (((sel >> 4) & 3) == 0) {
        uint32_t i2 = (uint32_t)(rng.u64() % n);
        term(qc, i2, minus1);
        val = add(val, c.w[i2]);
      }
      term(qc, n, one);
      c.w.push_back(val);
    }
    end_row();
  }
  c.n = (uint32_t)c.w.size();
}

static int generate(unsigned log_m, unsigned n_public, uint64_t circuit_seed, uint64_t toxic_seed, int device, Generated &g) {
  if (log_m < 2 || log_m > 26 || n_public + 2 > (1u << log_m)) { set_error("bad synthetic geometry log_m=%u nPublic=%u", log_m, n_public); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  synth_circuit(g.circ, 1u << log_m, n_public, circuit_seed, circuit_seed);
  SplitMix64 rng(toxic_seed);
  g.tox.t = rng.fr(); g.tox.alfa = rng.fr(); g.tox.beta = rng.fr(); g.tox.gamma = rng.fr(); g.tox.delta = rng.fr();
  return setup_from_circuit(device, g);
}

}  // namespace zkr

using namespace zkr;

extern "C" {

int zkr_synth_set_shape(unsigned shape) {
  if (shape > 1) { set_error("unknown synthetic circuit shape %u", shape); return ZKR_ERR_ARG; }
  g_shape = shape;
  return 0;
}

int zkr_synth_key(unsigned log_m, unsigned n_public, uint64_t circuit_seed, uint64_t toxic_seed, int device, zkr_key **key_out,
                  void **witness_out, size_t *witness_len, void **aux_out, size_t *aux_len) {
  if (!key_out || !witness_out || !witness_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  Generated g;
  int rc = generate(log_m, n_public, circuit_seed, toxic_seed, device, g);
  if (rc) return rc;
  rc = build_key_from_generated(g, device, key_out);
  if (rc) return rc;
  if ((rc = key_build_eval_tables(*key_out, g, false))) { zkr_key_free(*key_out); *key_out = nullptr; return rc; }
  // the witness, and the aux blob where it is asked for; the caller gets all of them or none
  std::vector<uint8_t> wb, aux;
  to_std_bytes(g.circ.w, wb);
  rc = give_bytes(wb, witness_out, witness_len);
  if (!rc && aux_out && aux_len) {
    const uint64_t n64 = g.circ.n;
    aux.assign((const uint8_t *)&n64, (const uint8_t *)&n64 + 8);
    std::vector<uint8_t> part;
    const std::vector<Fr> tv = {g.tox.t, g.tox.alfa, g.tox.beta, g.tox.gamma, g.tox.delta};
    const std::vector<Fr> *scalars[4] = {&tv, &g.sc.a, &g.sc.b, &g.sc.c};
    for (const std::vector<Fr> *v : scalars) {
      to_std_bytes(*v, part);
      aux.insert(aux.end(), part.begin(), part.end());
    }
    aux.insert(aux.end(), g.ic_std.begin(), g.ic_std.end());
    aux.insert(aux.end(), g.gamma2_std.begin(), g.gamma2_std.end());
    if ((rc = give_bytes(aux, aux_out, aux_len))) { free(*witness_out); *witness_out = nullptr; }
  }
  if (rc) { zkr_key_free(*key_out); *key_out = nullptr; }
  return rc;
}

int zkr_synth_witness(unsigned log_m, unsigned n_public, uint64_t circuit_seed, uint64_t witness_seed, void **witness_out, size_t *witness_len) {
  if (!witness_out || !witness_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (log_m < 2 || log_m > 26 || n_public + 2 > (1u << log_m)) { set_error("bad synthetic geometry"); return ZKR_ERR_ARG; }
  Circuit c;
  synth_circuit(c, 1u << log_m, n_public, circuit_seed, witness_seed);
  std::vector<uint8_t> wb;
  to_std_bytes(c.w, wb);
  return give_bytes(wb, witness_out, witness_len);
}

// verifying key of a synthetic key in the vk_bin layout of zkr_verify: alfa_1, beta_2, delta_2 from the key header
// (Montgomery there), gamma_2 and the IC points from the checker blob of zkr_synth_key
int zkr_synth_vk(const zkr_key *key, const void *aux, size_t aux_len, void **vk_out, size_t *vk_len) {
  if (!key || !aux || !vk_out || !vk_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  const uint8_t *ax = (const uint8_t *)aux;
  uint64_t n64 = 0;
  if (aux_len >= 8) memcpy(&n64, ax, 8);
  const size_t nic = (size_t)key->h.p + 1, ic_off = 8 + 160 + 96 * (size_t)n64;
  if (n64 != key->h.n || aux_len != ic_off + 64 * nic + 128) { set_error("aux blob does not belong to this key"); return ZKR_ERR_ARG; }
  std::vector<uint8_t> vk;
  write_vk(vk, key->h.alfa1, key->h.beta2, ax + ic_off + 64 * nic, key->h.delta2, ax + ic_off, nic);
  return give_bytes(vk, vk_out, vk_len);
}

int zkr_synth_websnark(unsigned log_m, unsigned n_public, uint64_t circuit_seed, uint64_t toxic_seed, int device, void **pk_out, size_t *pk_len,
                       void **witness_out, size_t *witness_len) {
  if (!pk_out || !pk_len || !witness_out || !witness_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  Generated g;
  int rc = generate(log_m, n_public, circuit_seed, toxic_seed, device, g);
  if (!rc) rc = render_websnark(g, pk_out, pk_len);
  if (rc) return rc;
  std::vector<uint8_t> wb;
  to_std_bytes(g.circ.w, wb);
  if ((rc = give_bytes(wb, witness_out, witness_len))) { free(*pk_out); *pk_out = nullptr; }
  return rc;
}

}  // extern "C"
