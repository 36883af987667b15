// websnark_writer.cpp -- the websnark proving-key layout (binarify.ts:143-206) as arithmetic and as a writer; host only, no HIP.
// zkr_websnark_len and zkr_websnark_render_host (include/zkr.h) are the two on their own; zkr_key_export.hip uses the same plan
// and the same front writer for a device key.
#include "websnark_writer.hpp"
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/zkr.h"

namespace zkr {
void set_error(const char *fmt, ...);

int websnark_plan(uint64_t n, uint64_t p, uint64_t m, uint64_t nnz_a, uint64_t nnz_b, WebsnarkPlan &pl) {
  const uint64_t lim = 0xffffffffull;
  if (n == 0 || n > lim || p >= n || m < 2 || m > lim || (m & (m - 1)) || nnz_a > lim || nnz_b > lim) {
    set_error("bad key geometry nVars=%llu nPublic=%llu domainSize=%llu", (unsigned long long)n, (unsigned long long)p, (unsigned long long)m);
    return ZKR_ERR_ARG;
  }
  pl.count[0] = pl.count[1] = pl.count[2] = n;
  pl.count[3] = n - p - 1;
  pl.count[4] = m;
  uint64_t off = 40 + 448, at[7];  // every term below is under 2^39: the sum cannot wrap
  at[0] = off; off += 4 * n + 36 * nnz_a;
  at[1] = off; off += 4 * n + 36 * nnz_b;
  for (int t = 0; t < 5; t++) { at[2 + t] = off; off += pl.count[t] * WEBSNARK_POINT_BYTES[t]; }
  if (off > lim) { set_error("websnark format is limited to 4 GiB (u32 offsets, binarify.ts:155-161)"); return ZKR_ERR_ARG; }
  for (int i = 0; i < 7; i++) pl.ptr[i] = (uint32_t)at[i];
  pl.len = off;
  return 0;
}

int websnark_write_front(uint8_t *o, const WebsnarkPlan &pl, uint32_t n, uint32_t p, uint32_t m, const uint8_t *consts448, const uint32_t *const rowptr[2],
                         const uint32_t *const col[2], const uint8_t *const coef[2]) {
  const uint32_t head[3] = {n, p, m};
  memcpy(o, head, 12);
  memcpy(o + 12, pl.ptr, 28);
  memcpy(o + 40, consts448, 448);
  std::vector<uint64_t> cur(n);
  for (int s = 0; s < 2; s++) {
    const uint64_t sec = pl.ptr[s], nnz = ((uint64_t)pl.ptr[s + 1] - sec - 4ull * n) / 36;
    const uint32_t *rp = rowptr[s];
    if (rp[0] != 0 || rp[m] != nnz) { set_error("side %d: row pointers run from %u to %u, not from 0 to %llu", s, rp[0], rp[m], (unsigned long long)nnz); return ZKR_ERR_ARG; }
    for (uint32_t r = 0; r < m; r++)
      if (rp[r] > rp[r + 1]) { set_error("side %d: row pointers descend at row %u", s, r); return ZKR_ERR_ARG; }
    // terms per signal, then where each signal's list starts
    std::fill(cur.begin(), cur.end(), 0);
    for (uint64_t e = 0; e < nnz; e++) {
      if (col[s][e] >= n) { set_error("side %d: term %llu names signal %u of %u", s, (unsigned long long)e, col[s][e], n); return ZKR_ERR_ARG; }
      cur[col[s][e]]++;
    }
    uint64_t at = sec;
    for (uint32_t sig = 0; sig < n; sig++) {
      const uint32_t k = (uint32_t)cur[sig];
      memcpy(o + at, &k, 4);
      cur[sig] = at + 4;
      at += 4 + 36ull * k;
    }
    // rows ascending: every list comes out by constraint index, terms of one row in the order they are stored
    for (uint32_t r = 0; r < m; r++)
      for (uint32_t e = rp[r]; e < rp[r + 1]; e++) {
        uint64_t &c = cur[col[s][e]];
        memcpy(o + c, &r, 4);
        memcpy(o + c + 4, coef[s] + (size_t)e * 32, 32);
        c += 36;
      }
  }
  return 0;
}

}  // namespace zkr

using namespace zkr;

extern "C" int zkr_websnark_len(uint64_t n_vars, uint64_t n_public, uint64_t domain, uint64_t nnz_a, uint64_t nnz_b, uint64_t *len) {
  if (!len) { set_error("null argument"); return ZKR_ERR_ARG; }
  WebsnarkPlan pl;
  if (int rc = websnark_plan(n_vars, n_public, domain, nnz_a, nnz_b, pl)) return rc;
  *len = pl.len;
  return 0;
}

extern "C" int zkr_websnark_render_host(uint32_t n_vars, uint32_t n_public, uint32_t domain, const uint8_t *consts448, const uint32_t *rowptr_a,
                                        const uint32_t *col_a, const uint8_t *coef_a, const uint32_t *rowptr_b, const uint32_t *col_b, const uint8_t *coef_b,
                                        const uint8_t *const points[5], void **pk_out, size_t *pk_len) {
  if (!consts448 || !rowptr_a || !rowptr_b || !points || !pk_out || !pk_len) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (domain == 0xffffffffu) { set_error("bad key geometry domainSize=%u", domain); return ZKR_ERR_ARG; }
  const uint32_t nnz_a = rowptr_a[domain], nnz_b = rowptr_b[domain];  // checked against the rows in websnark_write_front
  if ((nnz_a && (!col_a || !coef_a)) || (nnz_b && (!col_b || !coef_b))) { set_error("null argument"); return ZKR_ERR_ARG; }
  WebsnarkPlan pl;
  if (int rc = websnark_plan(n_vars, n_public, domain, nnz_a, nnz_b, pl)) return rc;
  for (int t = 0; t < 5; t++)
    if (pl.count[t] && !points[t]) { set_error("null argument"); return ZKR_ERR_ARG; }
  uint8_t *o = (uint8_t *)malloc(pl.len);
  if (!o) { set_error("no host memory for %llu bytes", (unsigned long long)pl.len); return ZKR_ERR_ARG; }
  const uint32_t *rp[2] = {rowptr_a, rowptr_b}, *cl[2] = {col_a, col_b};
  const uint8_t *cf[2] = {coef_a, coef_b};
  if (int rc = websnark_write_front(o, pl, n_vars, n_public, domain, consts448, rp, cl, cf)) { free(o); return rc; }
  for (int t = 0; t < 5; t++)
    if (pl.count[t]) memcpy(o + pl.ptr[2 + t], points[t], pl.count[t] * WEBSNARK_POINT_BYTES[t]);
  *pk_out = o;
  *pk_len = pl.len;
  return 0;
}
