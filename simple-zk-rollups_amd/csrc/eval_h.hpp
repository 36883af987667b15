// eval_h.hpp -- the scalars of a key's evaluation-form side tables (DESIGN.md 3.1 "H in evaluation form").  Nothing of HIP in it:
// the setups (zkr_setup.hip) call it where they hold the key's scalars, the host shim compiles it for the CPU tests.
//
// The H multiexp is linear in h, and h = (P - Q)/2 in coefficients, where P interpolates c_j = a_j b_j on the domain w^j and Q
// interpolates d_j = A(g w^j) B(g w^j) on the coset (g = w_2m, so x^m = -1 there).  Moving both inverse transforms from the
// scalars to the points:
//   sum_i h_i hx_i = 1/2 sum_j c_j f_j - 1/2 sum_j d_j e_j,   f_j = 1/m sum_i w^(-ij) hx_i,   e_j = 1/m sum_i (g w^j)^(-i) hx_i.
// For a witness that satisfies the R1CS c = C w, so the first sum folds into the C query: cfold_s = c_s + 1/2 sum_j C_js f_j
// (every signal, the public ones too).  The prover's coset evaluations come out of its unscaled inverse transforms as m ao_j and
// m bo_j in standard form, and one Montgomery product of the two leaves d'_j = m^2 d_j / R: eprime_j = -1/2 e_j R / m^2 makes
// sum_j d'_j eprime_j the second sum with nothing left to do per proof.
#pragma once
#include <stdint.h>
#include <vector>
#include "field.hpp"

namespace zkr {

// w_{2^k} in Montgomery form: 5^((r-1)/2^k) (5 = smallest quadratic non-residue mod r)
inline Fr fr_root_of_unity(unsigned k) {
  Fr five = Fr::zero();
  five.v[0] = 5;
  Fr g = to_mont(five);
  uint32_t e[8];
  for (int i = 0; i < 8; i++) e[i] = FrParams::P[i];
  e[0] -= 1;
  // e >>= 28
  for (int i = 0; i < 8; i++) e[i] = (e[i] >> 28) | (i < 7 ? e[i + 1] << 4 : 0);
  Fr r = Fr::one(), b = g;
  for (int i = 0; i < 256; i++) {
    if ((e[i >> 5] >> (i & 31)) & 1) r = mul(r, b);
    b = sqr(b);
  }
  for (unsigned j = k; j < 28; j++) r = sqr(r);
  return r;
}

// x[j] <- sum_i x[i] w^(ij) over the 2^logn-th roots of unity, natural order in and out; inverse: w^(-ij) and the factor 1/2^logn
inline void host_ntt(std::vector<Fr> &x, unsigned logn, bool inverse) {
  const size_t n = (size_t)1 << logn;
  if (n < 2) return;
  for (size_t i = 0; i < n; i++) {
    size_t j = 0;
    for (unsigned b = 0; b < logn; b++) j |= ((i >> b) & 1) << (logn - 1 - b);
    if (i < j) { Fr t = x[i]; x[i] = x[j]; x[j] = t; }
  }
  Fr w = fr_root_of_unity(logn);
  if (inverse) w = inv(w);
  std::vector<Fr> tw(n / 2);
  Fr cur = Fr::one();
  for (size_t i = 0; i < n / 2; i++) { tw[i] = cur; cur = mul(cur, w); }
  for (unsigned s = 0; s < logn; s++) {
    const size_t half = (size_t)1 << s, step = n >> (s + 1);
    for (size_t blk = 0; blk < n; blk += 2 * half)
      for (size_t i = 0; i < half; i++) {
        const Fr u = x[blk + i], v = mul(x[blk + half + i], tw[i * step]);
        x[blk + i] = add(u, v);
        x[blk + half + i] = sub(u, v);
      }
  }
  if (inverse) {
    Fr nn = Fr::zero();
    nn.v[0] = (uint32_t)n; nn.v[1] = (uint32_t)((uint64_t)n >> 32);
    const Fr ninv = inv(to_mont(nn));
    for (size_t i = 0; i < n; i++) x[i] = mul(x[i], ninv);
  }
}

struct EvalHScalars {
  std::vector<Fr> f, e;    // the two transforms of hx, natural order (Montgomery, like everything here)
  std::vector<Fr> cfold;   // n: the scalar of signal s in the folded C table
  std::vector<Fr> eprime;  // m: the scalar of coset position j in the E table, every constant folded in
};
// hx: the m scalars of the H table (power i at index i); C by constraint row (rowC: nC + 1 row pointers into sigC / coefC); cpriv:
// the scalars of the plain C query, signal p + 1 + i at index i
inline void eval_h_scalars(const Fr *hx, unsigned logm, const uint32_t *rowC, const uint32_t *sigC, const Fr *coefC, uint32_t nC, uint32_t n, uint32_t p,
                           const Fr *cpriv, EvalHScalars &out) {
  const size_t m = (size_t)1 << logm;
  out.f.assign(hx, hx + m);
  host_ntt(out.f, logm, true);
  out.e.resize(m);
  const Fr ginv = inv(fr_root_of_unity(logm + 1));
  Fr gi = Fr::one();
  for (size_t i = 0; i < m; i++) { out.e[i] = mul(hx[i], gi); gi = mul(gi, ginv); }
  host_ntt(out.e, logm, true);
  Fr two = Fr::zero(), mm = Fr::zero();
  two.v[0] = 2;
  mm.v[0] = (uint32_t)m; mm.v[1] = (uint32_t)((uint64_t)m >> 32);
  const Fr half = inv(to_mont(two)), minv = inv(to_mont(mm));
  std::vector<Fr> acc(n, Fr::zero());
  for (uint32_t j = 0; j < nC; j++)
    for (uint32_t k = rowC[j]; k < rowC[j + 1]; k++) acc[sigC[k]] = add(acc[sigC[k]], mul(coefC[k], out.f[j]));
  out.cfold.resize(n);
  for (uint32_t s = 0; s < n; s++) {
    const Fr fold = mul(acc[s], half);
    out.cfold[s] = s > p ? add(cpriv[s - p - 1], fold) : fold;
  }
  // Fr::r2() is the field element R in Montgomery form
  const Fr ke = neg(mul(mul(half, Fr::r2()), mul(minv, minv)));
  out.eprime.resize(m);
  for (size_t j = 0; j < m; j++) out.eprime[j] = mul(out.e[j], ke);
}

}  // namespace zkr
