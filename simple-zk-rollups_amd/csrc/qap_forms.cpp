// qap_forms.cpp -- the parsers and conversions of qap_forms.hpp; host only, no HIP.  Both parsers read untrusted bytes:
// `make qap-asan` runs qap_forms_selfcheck.cpp over this unit under AddressSanitizer and UBSan.
#include "qap_forms.hpp"
#include <string.h>
#include "../../include/zkr.h"

namespace zkr {
void set_error(const char *fmt, ...);

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

int parse_r1cs(const void *r1cs_bin, size_t r1cs_len, Circuit &c) {
  const uint8_t *b = (const uint8_t *)r1cs_bin, *end = b + r1cs_len;
  if (r1cs_len < 12) { set_error("R1CS shorter than its header"); return ZKR_ERR_ARG; }
  memcpy(&c.n, b, 4); memcpy(&c.p, b + 4, 4); memcpy(&c.nC, b + 8, 4);
  b += 12;
  if (c.n < 1 || (uint64_t)c.p + 1 > c.n || c.nC < 1 || (uint64_t)c.nC + c.p + 1 > (1ull << 26)) { set_error("bad R1CS geometry nVars=%u nPublic=%u nConstraints=%u", c.n, c.p, c.nC); return ZKR_ERR_ARG; }
  c.m = 2;
  while (c.m < c.nC + c.p + 1) c.m <<= 1;  // snarkjs: domainBits = floor(log2(nC + nPublic)) + 1
  for (QapRows &q : c.side) q.rowptr.push_back(0);
  for (uint32_t row = 0; row < c.nC; row++) {
    for (QapRows &q : c.side) {
      if (b + 4 > end) { set_error("R1CS truncated in constraint %u", row); return ZKR_ERR_ARG; }
      uint32_t k;
      memcpy(&k, b, 4);
      b += 4;
      if ((uint64_t)k * 36 > (uint64_t)(end - b)) { set_error("R1CS truncated in constraint %u", row); return ZKR_ERR_ARG; }
      for (uint32_t e = 0; e < k; e++, b += 36) {
        const uint32_t sig = rd32(b);
        Fr cf;
        if (sig >= c.n || !read_fr_std(b + 4, cf)) { set_error("constraint %u: signal %u out of range or coefficient >= r", row, sig); return ZKR_ERR_ARG; }
        q.sig.push_back(sig);
        q.coef.push_back(to_mont(cf));
      }
      q.rowptr.push_back((uint32_t)q.sig.size());
    }
  }
  if (b != end) { set_error("R1CS has %zu trailing bytes", (size_t)(end - b)); return ZKR_ERR_ARG; }
  return 0;
}

void key_rows(const Circuit &c, int side, bool standard, KeyRows &out) {
  const QapRows &q = c.side[side];
  const size_t nnz = q.sig.size(), extra = side == 0 ? (size_t)c.p + 1 : 0;
  out.col = q.sig;
  out.col.resize(nnz + extra);
  out.coef.resize((nnz + extra) * 32);
  for (size_t e = 0; e < nnz; e++) {
    const Fr v = standard ? from_mont(q.coef[e]) : q.coef[e];
    memcpy(&out.coef[e * 32], v.v, 32);
  }
  const Fr one = standard ? from_mont(Fr::one()) : Fr::one();
  for (size_t i = 0; i < extra; i++) {
    out.col[nnz + i] = (uint32_t)i;
    memcpy(&out.coef[(nnz + i) * 32], one.v, 32);
  }
  out.rowptr.resize((size_t)c.m + 1);
  for (uint32_t r = 0; r <= c.m; r++) {
    const uint32_t past = r > c.nC ? r - c.nC : 0;  // input-consistency rows before row r
    out.rowptr[r] = q.rowptr[r < c.nC ? r : c.nC] + (uint32_t)(past < extra ? past : extra);
  }
}

void qap_columns(const Circuit &c, int side, QapColumns &q) {
  KeyRows rows;
  key_rows(c, side, true, rows);
  q.colptr.assign((size_t)c.n + 1, 0);
  for (uint32_t sig : rows.col) q.colptr[sig + 1]++;
  for (uint32_t s = 0; s < c.n; s++) q.colptr[s + 1] += q.colptr[s];
  q.row.resize(rows.col.size());
  q.coef.resize(rows.coef.size());
  std::vector<uint32_t> fill(q.colptr.begin(), q.colptr.end() - 1);
  for (uint32_t r = 0; r < c.m; r++)
    for (uint32_t e = rows.rowptr[r]; e < rows.rowptr[r + 1]; e++) {
      const uint32_t at = fill[rows.col[e]]++;
      q.row[at] = r;
      memcpy(&q.coef[(size_t)at * 32], &rows.coef[(size_t)e * 32], 32);
    }
}

int pols_to_rows(const uint8_t *pk, size_t begin, size_t end, int s, uint32_t n, uint32_t m, KeyRows &out) {
  size_t o = begin;
  std::vector<uint32_t> cnt((size_t)m + 1, 0);
  size_t nnz = 0;
  for (uint32_t sig = 0; sig < n; sig++) {
    if (o + 4 > end) { set_error("pols section %d truncated", s); return ZKR_ERR_BAD_KEY; }
    uint32_t kk = rd32(pk + o);
    o += 4;
    if (o + 36ull * kk > end) { set_error("pols section %d truncated", s); return ZKR_ERR_BAD_KEY; }
    for (uint32_t e = 0; e < kk; e++, o += 36) {
      uint32_t c = rd32(pk + o);
      if (c >= m) { set_error("constraint index %u >= domainSize %u", c, m); return ZKR_ERR_BAD_KEY; }
      cnt[c + 1]++;
    }
    nnz += kk;
  }
  if (o != end) { set_error("pols section %d has trailing bytes", s); return ZKR_ERR_BAD_KEY; }
  out.rowptr.assign((size_t)m + 1, 0);
  for (uint32_t c = 0; c < m; c++) out.rowptr[c + 1] = out.rowptr[c] + cnt[c + 1];
  out.col.resize(nnz);
  out.coef.resize(nnz * 32);
  std::vector<uint32_t> cur(out.rowptr.begin(), out.rowptr.end() - 1);
  o = begin;
  for (uint32_t sig = 0; sig < n; sig++) {
    uint32_t kk = rd32(pk + o);
    o += 4;
    for (uint32_t e = 0; e < kk; e++, o += 36) {
      uint32_t c = rd32(pk + o), pos = cur[c]++;
      out.col[pos] = sig;
      memcpy(&out.coef[(size_t)pos * 32], pk + o + 4, 32);
    }
  }
  return 0;
}

}  // namespace zkr
