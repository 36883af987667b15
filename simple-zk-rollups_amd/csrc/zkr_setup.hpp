// zkr_setup.hpp -- what a finished Groth16 setup holds (zkr_setup.hip), for the entry points that run one: the zkr_setup_r1cs*
// calls there and the zkr_synth_* calls of workload.hip.
#pragma once
#include "zkr_internal.hpp"

namespace zkr {

inline Fr fr_u64(uint64_t x) {
  Fr r = Fr::zero();
  r.v[0] = (uint32_t)x;
  r.v[1] = (uint32_t)(x >> 32);
  return to_mont(r);
}
inline void to_std_bytes(const std::vector<Fr> &v, std::vector<uint8_t> &out) {
  out.resize(v.size() * 32);
  for (size_t i = 0; i < v.size(); i++) { Fr s = from_mont(v[i]); memcpy(&out[i * 32], s.v, 32); }
}
template <class T>
inline void wipe_vector(std::vector<T> &v) {
  if (!v.empty()) explicit_bzero((void *)v.data(), v.size() * sizeof(T));
}

struct Toxic { Fr t, alfa, beta, gamma, delta; };  // Montgomery

struct SetupScalars {
  std::vector<Fr> a, b, c;            // per signal, Montgomery
  std::vector<Fr> cpriv, ic, hx;      // (beta a + alfa b + c)/delta for s>p ; /gamma for s<=p ; t^i Z(t)/delta
};

struct Generated {
  Circuit circ;
  Toxic tox;
  SetupScalars sc;
  bool secret = false;  // fresh toxic waste (zkr_setup_r1cs without injected scalars): everything derived from it is wiped
  DevBuf d_tbl[N_TABLES];
  uint8_t consts[448];
  std::vector<uint8_t> ic_std, gamma2_std;
  ~Generated() {
    if (secret) {  // t, alfa, beta, gamma, delta and the per-signal / per-power scalars (a_s, b_s, c_s, K_s/delta, K_s/gamma, t^i Z/delta):
                   // any of them lets its holder forge proofs for the generated key
      explicit_bzero((void *)&tox, sizeof(tox));
      wipe_vector(sc.a); wipe_vector(sc.b); wipe_vector(sc.c); wipe_vector(sc.cpriv); wipe_vector(sc.ic); wipe_vector(sc.hx);
    }
  }
};

int setup_from_circuit(int device, Generated &g);  // g.circ and g.tox are in place: QAP polynomials at t, then every group element of the key on the GPU
int build_key_from_generated(const Generated &g, int device, zkr_key **key_out);
int key_build_eval_tables(zkr_key *k, const Generated &g, bool refuse);  // the side tables of H in evaluation form from the setup's own scalars
int render_websnark(const Generated &g, void **pk_out, size_t *pk_len);  // the key in the byte layout binarifyProvingKey writes
int vk_to_malloc(const Generated &g, void **vk_out, size_t *vk_len);     // vk_bin (zkr_verify layout) from the setup's own data

}  // namespace zkr
