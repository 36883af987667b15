// qap_forms.hpp -- the forms a circuit's QAP takes on the host, each written once; no HIP in it or in qap_forms.cpp.
//   Circuit     a rank-1 constraint system as parse_r1cs reads it: three sides by constraint row, struct of arrays, Montgomery
//               coefficients -- what zkr_r1cs.hip uploads and eval_h_scalars reads, by pointer
//   KeyRows     one side AS A KEY HOLDS IT (key_rows): by row over the whole domain, A with the nPublic + 1 input-consistency rows
//               snarkjs appends, coefficients as bytes -- the arena's A and B, C of the evaluation form, the websnark front writer
//   QapColumns  the same by signal, rows ascending, standard form (qap_columns): what the powers-of-tau setup combines points with
//   pols_to_rows  the way back: a websnark pols section (by signal) -> KeyRows
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include <vector>
#include "field.hpp"

namespace zkr {

// A QAP row of more terms than this goes to a wavefront of its own: kernels_ntt.hpp SPMV_WIDE and zkr_r1cs.hip R1CS_WIDE are this
constexpr uint32_t WIDE_ROW_TERMS = 8;
// the rows < `rows` that are wider than `threshold` in one of the CSR sides given, ascending
inline std::vector<uint32_t> wide_rows(std::initializer_list<const uint32_t *> rowptr, uint32_t rows, uint32_t threshold = WIDE_ROW_TERMS) {
  std::vector<uint32_t> wide;
  for (uint32_t r = 0; r < rows; r++)
    for (const uint32_t *rp : rowptr)
      if (rp[r + 1] - rp[r] > threshold) { wide.push_back(r); break; }
  return wide;
}
inline std::vector<uint32_t> wide_rows(const uint32_t *rowptr, uint32_t rows, uint32_t threshold = WIDE_ROW_TERMS) { return wide_rows({rowptr}, rows, threshold); }

inline unsigned domain_log2(uint32_t m) {  // the least k with 2^k >= m
  unsigned k = 0;
  while ((1u << k) < m) k++;
  return k;
}
inline uint32_t bitrev32(uint32_t x, unsigned bits) {
  uint32_t r = 0;
  for (unsigned b = 0; b < bits; b++) r |= ((x >> b) & 1) << (bits - 1 - b);
  return r;
}

inline bool read_fr_std(const uint8_t *p, Fr &out) {  // 32 standard-form bytes; false: not below r
  memcpy(out.v, p, 32);
  return words_below(out.v, FrParams::P);
}

struct QapRows {  // one side by constraint: row r = the terms [rowptr[r], rowptr[r + 1])
  std::vector<uint32_t> rowptr, sig;  // nConstraints + 1 row pointers; signal per term
  std::vector<Fr> coef;               // Montgomery
};
struct Circuit {
  uint32_t n = 0, p = 0, nC = 0, m = 0;
  QapRows side[3];    // A, B, C
  std::vector<Fr> w;  // Montgomery
};
// r1cs_bin (include/zkr.h) -> the circuit, with its domain; ZKR_ERR_ARG with a message
int parse_r1cs(const void *r1cs_bin, size_t r1cs_len, Circuit &c);

struct KeyRows {
  std::vector<uint32_t> rowptr, col;  // m + 1 row pointers; signal per term
  std::vector<uint8_t> coef;          // 32 B per term
};
// side 0 = A with its input-consistency rows (row nC + i: signal i, coefficient one, i <= nPublic), 1 = B, 2 = C; rows from
// there on are empty.  Terms in stored order, nothing merged or dropped; coefficients Montgomery, or standard form
void key_rows(const Circuit &c, int side, bool standard, KeyRows &out);

// One QAP matrix by signal: column s = the terms [colptr[s], colptr[s + 1]), term e = coef[32 e ..] (standard form) x L_row[e]
struct QapColumns {
  std::vector<uint32_t> colptr, row;
  std::vector<uint8_t> coef;
};
void qap_columns(const Circuit &c, int side, QapColumns &q);  // key_rows(side) by signal, rows ascending

// pk[begin, end): pols section s of a websnark proving key (per signal a u32 count, then (u32 row, 32 B coefficient) pairs; the
// caller has checked begin <= end <= the buffer's length) -> rows over the domain m, coefficients as they are.  ZKR_ERR_BAD_KEY
// with a message: the section is truncated, has trailing bytes, or names a row >= m
int pols_to_rows(const uint8_t *pk, size_t begin, size_t end, int s, uint32_t n, uint32_t m, KeyRows &out);

}  // namespace zkr
