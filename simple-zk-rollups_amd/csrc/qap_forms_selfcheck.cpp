// qap_forms_selfcheck.cpp -- a stand-alone program over qap_forms.cpp (the circuit, its forms as a key holds them, the two parsers
// of untrusted bytes) meant for a sanitizer build (`make qap-asan`: AddressSanitizer + UBSan on this file, qap_forms.cpp and
// websnark_writer.cpp; no Python and no HIP in the process).  The reference is the code these forms replaced, kept here as it
// was: terms as an array of structs that every consumer split again by hand, the input-consistency rows appended in each place,
// and the websnark writer over one vector of (row, coefficient) pairs per signal.  Seeded small circuits at the sizes where the
// forms can go wrong, then a few hundred damaged buffers for each parser: every one is refused, in the words the callers had.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>

#include "../../include/zkr.h"
#include "qap_forms.hpp"
#include "websnark_writer.hpp"

static char last_error[256];
namespace zkr {
void set_error(const char *fmt, ...) {  // the library's lives beside its HIP code
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof(last_error), fmt, ap);
  va_end(ap);
}
}  // namespace zkr
extern "C" void zkr_free(void *p) { free(p); }  // as the library's (websnark_writer.cpp's host renderer hands out malloc'ed bytes)
using namespace zkr;

static int fails = 0, refusals = 0;
#define CHECK(x) do { if (!(x)) { fails++; fprintf(stderr, "line %d: %s\n", __LINE__, #x); } } while (0)

static uint64_t rng_state = 0x51A90001;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static void put32(std::vector<uint8_t> &o, uint32_t v) { o.insert(o.end(), (const uint8_t *)&v, (const uint8_t *)&v + 4); }
static std::string fmt(const char *f, ...) {
  char b[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(b, sizeof(b), f, ap);
  va_end(ap);
  return b;
}
// the bytes in a heap block of exactly their length: a read one past it is the sanitizer's to find
struct Exact {
  uint8_t *p;
  size_t len;
  explicit Exact(const std::vector<uint8_t> &v, size_t n) : p((uint8_t *)malloc(n ? n : 1)), len(n) { if (n) memcpy(p, v.data(), n); }
  ~Exact() { free(p); }
  Exact(const Exact &) = delete;
};

// ---- the reference: the circuit as it was held, and the loops that split it
struct Term { uint32_t sig; Fr coef; };  // coef Montgomery
struct OldCircuit {
  uint32_t n = 0, p = 0, nC = 0, m = 0;
  std::vector<uint32_t> row[3];  // nC + 1 row pointers
  std::vector<Term> t[3];
};

static Fr rnd_fr_std() {
  Fr v;
  for (int i = 0; i < 8; i += 2) { uint64_t x = rnd(); v.v[i] = (uint32_t)x; v.v[i + 1] = (uint32_t)(x >> 32); }
  v.v[7] &= 0x1fffffffu;  // below 2^253 < r
  return v;
}

// wild 1: a (row, signal) pair stored twice; 2: zero coefficients; rows 0 and 1 of A get 8 and 9 terms, row 2 of every side none,
// the last signal never gets a term (n > 1)
static void draw(OldCircuit &c, std::vector<uint8_t> &r1cs, std::vector<size_t> &bounds, uint32_t n, uint32_t p, uint32_t nC, unsigned wild) {
  c.n = n; c.p = p; c.nC = nC;
  c.m = 2;
  while (c.m < nC + p + 1) c.m <<= 1;
  put32(r1cs, n); put32(r1cs, p); put32(r1cs, nC);
  for (int s = 0; s < 3; s++) c.row[s].push_back(0);
  for (uint32_t r = 0; r < nC; r++)
    for (int s = 0; s < 3; s++) {
      uint32_t k = (uint32_t)(rnd() % 4);
      if (s == 0 && r < 2) k = 8 + r;
      if (r == 2) k = 0;
      bounds.push_back(r1cs.size());
      put32(r1cs, k);
      for (uint32_t e = 0; e < k; e++) {
        uint32_t sig = (uint32_t)(rnd() % (n > 1 ? n - 1 : 1));
        if ((wild & 1) && e) sig = c.t[s].back().sig;
        Fr cf = rnd_fr_std();
        if ((wild & 2) && rnd() % 3 == 0) cf = Fr::zero();
        bounds.push_back(r1cs.size());
        put32(r1cs, sig);
        r1cs.insert(r1cs.end(), (const uint8_t *)cf.v, (const uint8_t *)cf.v + 32);
        c.t[s].push_back(Term{sig, to_mont(cf)});
      }
      c.row[s].push_back((uint32_t)c.t[s].size());
    }
  bounds.push_back(r1cs.size());
}

// A and B for the arena (the setup's build_key_from_tables): Montgomery bytes, A with the input-consistency rows
static void old_arena_rows(const OldCircuit &c, int s, KeyRows &o) {
  o.rowptr.assign(c.m + 1, 0);
  for (uint32_t r = 0; r < c.m; r++) {
    o.rowptr[r] = (uint32_t)o.col.size();
    if (r < c.nC) {
      for (uint32_t k = c.row[s][r]; k < c.row[s][r + 1]; k++) {
        o.col.push_back(c.t[s][k].sig);
        const uint8_t *b = (const uint8_t *)c.t[s][k].coef.v;
        o.coef.insert(o.coef.end(), b, b + 32);
      }
    } else if (s == 0 && r - c.nC <= c.p) {
      o.col.push_back(r - c.nC);
      Fr one = Fr::one();
      const uint8_t *b = (const uint8_t *)one.v;
      o.coef.insert(o.coef.end(), b, b + 32);
    }
  }
  o.rowptr[c.m] = (uint32_t)o.col.size();
}
// C by row for the evaluation form (key_eval_rows): standard form, row pointers padded to the domain
static void old_eval_rows(const OldCircuit &c, KeyRows &o) {
  o.col.resize(c.t[2].size());
  o.coef.resize(c.t[2].size() * 32);
  for (size_t i = 0; i < c.t[2].size(); i++) {
    o.col[i] = c.t[2][i].sig;
    Fr v = from_mont(c.t[2][i].coef);
    memcpy(&o.coef[i * 32], v.v, 32);
  }
  o.rowptr.resize(c.m + 1);
  for (uint32_t r = 0; r <= c.m; r++) o.rowptr[r] = c.row[2][r < c.nC ? r : c.nC];
}
static void old_qap_columns(const OldCircuit &c, int side, QapColumns &q) {
  const uint32_t n = c.n, p = c.p;
  const std::vector<uint32_t> &rp = c.row[side];
  const std::vector<Term> &tt = c.t[side];
  q.colptr.assign(n + 1, 0);
  for (const Term &t : tt) q.colptr[t.sig + 1]++;
  if (side == 0) for (uint32_t i = 0; i <= p; i++) q.colptr[i + 1]++;
  for (uint32_t s = 0; s < n; s++) q.colptr[s + 1] += q.colptr[s];
  q.row.resize(q.colptr[n]);
  q.coef.resize((size_t)q.colptr[n] * 32);
  std::vector<uint32_t> fill(q.colptr.begin(), q.colptr.end() - 1);
  auto put = [&](uint32_t sig, uint32_t row, const Fr &coef_mont) {
    const uint32_t e = fill[sig]++;
    const Fr std_form = from_mont(coef_mont);
    q.row[e] = row;
    memcpy(&q.coef[(size_t)e * 32], std_form.v, 32);
  };
  for (uint32_t r = 0; r < c.nC; r++)
    for (uint32_t e = rp[r]; e < rp[r + 1]; e++) put(tt[e].sig, r, tt[e].coef);
  if (side == 0) for (uint32_t i = 0; i <= p; i++) put(i, c.nC + i, Fr::one());
}
// header and pols sections as the setup's own writer laid them out: one vector of (row, coefficient) per signal
static void old_websnark_front(const OldCircuit &c, const uint8_t *consts448, std::vector<uint8_t> &o) {
  const uint32_t n = c.n, p = c.p, m = c.m;
  std::vector<std::vector<std::pair<uint32_t, Fr>>> col[2];
  for (int s = 0; s < 2; s++) {
    col[s].resize(n);
    for (uint32_t r = 0; r < c.nC; r++)
      for (uint32_t k = c.row[s][r]; k < c.row[s][r + 1]; k++) col[s][c.t[s][k].sig].push_back({r, c.t[s][k].coef});
  }
  for (uint32_t i = 0; i <= p; i++) col[0][i].push_back({c.nC + i, Fr::one()});
  put32(o, n); put32(o, p); put32(o, m);
  const size_t ptr_at = o.size();
  o.resize(o.size() + 28);
  o.insert(o.end(), consts448, consts448 + 448);
  uint32_t ptrs[7];
  for (int s = 0; s < 2; s++) {
    ptrs[s] = (uint32_t)o.size();
    for (uint32_t sig = 0; sig < n; sig++) {
      put32(o, (uint32_t)col[s][sig].size());
      for (auto &e : col[s][sig]) { put32(o, e.first); o.insert(o.end(), (const uint8_t *)e.second.v, (const uint8_t *)e.second.v + 32); }
    }
  }
  const size_t counts[5] = {n, n, n, n - p - 1, m};
  size_t off = o.size();
  for (int t = 0; t < 5; t++) { ptrs[2 + t] = (uint32_t)off; off += counts[t] * WEBSNARK_POINT_BYTES[t]; }
  memcpy(&o[ptr_at], ptrs, 28);
}
// column-major pols -> rows, as the loader had it (its checks are pols_to_rows' own: the damaged buffers below)
static void old_pols_to_rows(const uint8_t *pk, size_t begin, uint32_t n, uint32_t m, KeyRows &out) {
  std::vector<uint32_t> cnt(m + 1, 0);
  size_t o = begin, nnz = 0;
  for (uint32_t sig = 0; sig < n; sig++) {
    uint32_t kk = rd32(pk + o);
    o += 4;
    for (uint32_t e = 0; e < kk; e++, o += 36) cnt[rd32(pk + o) + 1]++;
    nnz += kk;
  }
  out.rowptr.assign(m + 1, 0);
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
}

static bool same(const KeyRows &a, const KeyRows &b) { return a.rowptr == b.rowptr && a.col == b.col && a.coef == b.coef; }

// rc and message of a parse that must be refused
static void refused_r1cs(const std::vector<uint8_t> &bytes, size_t len, const std::string &want) {
  Exact e(bytes, len);
  Circuit c;
  last_error[0] = 0;
  const int rc = parse_r1cs(e.p, e.len, c);
  if (rc != ZKR_ERR_ARG || want != last_error) { fails++; fprintf(stderr, "parse_r1cs: rc %d \"%s\", expected \"%s\"\n", rc, last_error, want.c_str()); }
  refusals++;
}
static void refused_pols(const std::vector<uint8_t> &bytes, size_t len, size_t begin, size_t end, int s, uint32_t n, uint32_t m, const std::string &want) {
  Exact e(bytes, len);
  KeyRows rows;
  last_error[0] = 0;
  const int rc = pols_to_rows(e.p, begin, end, s, n, m, rows);
  if (rc != ZKR_ERR_BAD_KEY || want != last_error) { fails++; fprintf(stderr, "pols_to_rows: rc %d \"%s\", expected \"%s\"\n", rc, last_error, want.c_str()); }
  refusals++;
}

static void run(uint32_t n, uint32_t p, uint32_t nC, unsigned wild) {
  OldCircuit old;
  std::vector<uint8_t> r1cs;
  std::vector<size_t> bounds;  // where every count and every term starts, and the end
  draw(old, r1cs, bounds, n, p, nC, wild);
  const uint32_t m = old.m;

  // the circuit: the same terms, side by side instead of term by term
  Circuit c;
  {
    Exact e(r1cs, r1cs.size());
    CHECK(parse_r1cs(e.p, e.len, c) == 0);
  }
  CHECK(c.n == n && c.p == p && c.nC == nC && c.m == m);
  for (int s = 0; s < 3; s++) {
    CHECK(c.side[s].rowptr == old.row[s] && c.side[s].sig.size() == old.t[s].size() && c.side[s].coef.size() == old.t[s].size());
    for (size_t i = 0; i < old.t[s].size() && i < c.side[s].sig.size(); i++)
      CHECK(c.side[s].sig[i] == old.t[s][i].sig && !memcmp(c.side[s].coef[i].v, old.t[s][i].coef.v, 32));
  }
  // by row as the key holds them
  KeyRows now[2], was;
  for (int s = 0; s < 2; s++) {
    was = KeyRows();
    old_arena_rows(old, s, was);
    key_rows(c, s, false, now[s]);
    CHECK(same(now[s], was));
    // wide rows: the literal the three units each had
    std::vector<uint32_t> wide;
    for (uint32_t r = 0; r < m; r++)
      if (was.rowptr[r + 1] - was.rowptr[r] > 8) wide.push_back(r);
    CHECK(wide_rows(now[s].rowptr.data(), m) == wide);
    if (s == 0 && nC > 1) CHECK(wide == std::vector<uint32_t>{1});  // eight terms stay narrow, nine do not
  }
  {
    std::vector<uint32_t> wide;  // the R1CS check's: a constraint with any wide side
    for (uint32_t r = 0; r < nC; r++)
      if (old.row[0][r + 1] - old.row[0][r] > 8 || old.row[1][r + 1] - old.row[1][r] > 8 || old.row[2][r + 1] - old.row[2][r] > 8) wide.push_back(r);
    CHECK(wide_rows({c.side[0].rowptr.data(), c.side[1].rowptr.data(), c.side[2].rowptr.data()}, nC) == wide);
  }
  KeyRows ev;
  was = KeyRows();
  old_eval_rows(old, was);
  key_rows(c, 2, true, ev);
  CHECK(same(ev, was));
  // by signal
  for (int s = 0; s < 3; s++) {
    QapColumns qn, qo;
    old_qap_columns(old, s, qo);
    qap_columns(c, s, qn);
    CHECK(qn.colptr == qo.colptr && qn.row == qo.row && qn.coef == qo.coef);
  }
  // the websnark front: the per-signal writer against plan + front writer over the rows above
  uint8_t consts[448];
  for (uint8_t &b : consts) b = (uint8_t)rnd();
  std::vector<uint8_t> front_was, front_now;
  old_websnark_front(old, consts, front_was);
  WebsnarkPlan pl;
  CHECK(websnark_plan(n, p, m, now[0].col.size(), now[1].col.size(), pl) == 0);
  CHECK(pl.ptr[2] == front_was.size());
  front_now.assign(pl.ptr[2], 0xEE);
  const uint32_t *rp[2] = {now[0].rowptr.data(), now[1].rowptr.data()}, *cl[2] = {now[0].col.data(), now[1].col.data()};
  const uint8_t *cf[2] = {now[0].coef.data(), now[1].coef.data()};
  {
    Exact e(front_now, front_now.size());
    CHECK(websnark_write_front(e.p, pl, n, p, m, consts, rp, cl, cf) == 0);
    front_now.assign(e.p, e.p + e.len);
  }
  CHECK(front_now == front_was);
  if (front_now != front_was) return;
  // and back: the loader's pass over both sections
  const std::vector<uint8_t> &pk = front_was;
  const uint32_t ptr[3] = {rd32(&pk[12]), rd32(&pk[16]), rd32(&pk[20])};
  for (int s = 0; s < 2; s++) {
    KeyRows back;
    was = KeyRows();
    old_pols_to_rows(pk.data(), ptr[s], n, m, was);
    Exact e(pk, pk.size());
    CHECK(pols_to_rows(e.p, ptr[s], ptr[s + 1], s, n, m, back) == 0);
    CHECK(same(back, was) && back.rowptr == now[s].rowptr);
  }

  // ---- damaged R1CS buffers
  refused_r1cs(r1cs, 0, "R1CS shorter than its header");
  refused_r1cs(r1cs, 11, "R1CS shorter than its header");
  {  // every boundary: what lies before it is whole, the constraint it belongs to is named
    size_t bi = 0;
    for (uint32_t r = 0; r < nC; r++) {
      size_t in_row = 0;
      for (int s = 0; s < 3; s++) in_row += 1 + (old.row[s][r + 1] - old.row[s][r]);
      for (size_t k = 0; k < in_row; k++, bi++) {
        refused_r1cs(r1cs, bounds[bi], fmt("R1CS truncated in constraint %u", r));
        refused_r1cs(r1cs, bounds[bi] + 3, fmt("R1CS truncated in constraint %u", r));
      }
    }
    CHECK(bi + 1 == bounds.size());
  }
  {  // counts of 0xffffffff, one side at a time; a signal at the bound and one past it; a coefficient of r; trailing bytes; geometry
    size_t at = 12;
    for (uint32_t r = 0; r < nC; r++)
      for (int s = 0; s < 3; s++) {
        const uint32_t k = old.row[s][r + 1] - old.row[s][r];
        std::vector<uint8_t> bad = r1cs;
        const uint32_t all = 0xffffffffu;
        memcpy(&bad[at], &all, 4);
        refused_r1cs(bad, bad.size(), fmt("R1CS truncated in constraint %u", r));
        if (k) {
          bad = r1cs;
          memcpy(&bad[at + 4], &n, 4);
          refused_r1cs(bad, bad.size(), fmt("constraint %u: signal %u out of range or coefficient >= r", r, n));
          const uint32_t last = n - 1, keep = rd32(&r1cs[at + 4]);
          memcpy(&bad[at + 4], &last, 4);
          Exact e(bad, bad.size());
          Circuit ok;
          CHECK(parse_r1cs(e.p, e.len, ok) == 0 && ok.side[s].sig[old.row[s][r]] == last);
          bad = r1cs;
          memcpy(&bad[at + 8], FrParams::P, 32);
          refused_r1cs(bad, bad.size(), fmt("constraint %u: signal %u out of range or coefficient >= r", r, keep));
        }
        at += 4 + 36 * (size_t)k;
      }
    std::vector<uint8_t> bad = r1cs;
    for (size_t extra = 1; extra <= 5; extra += 4) {
      bad.resize(r1cs.size() + extra, 0);
      refused_r1cs(bad, bad.size(), fmt("R1CS has %zu trailing bytes", extra));
    }
    const uint32_t geometry[4][3] = {{0, 0, nC}, {n, n, nC}, {n, p, 0}, {n, p, (1u << 26) - p}};
    for (const uint32_t *g : geometry) {
      bad = r1cs;
      memcpy(&bad[0], g, 12);
      refused_r1cs(bad, bad.size(), fmt("bad R1CS geometry nVars=%u nPublic=%u nConstraints=%u", g[0], g[1], g[2]));
    }
  }
  // ---- damaged pols sections
  for (int s = 0; s < 2; s++) {
    const std::string cut = fmt("pols section %d truncated", s);
    size_t o = ptr[s];
    for (uint32_t sig = 0; sig < n; sig++) {  // the section ends at, or inside, every count and every term: the buffer ends there too
      const uint32_t kk = rd32(&pk[o]);
      refused_pols(pk, o, ptr[s], o, s, n, m, cut);
      refused_pols(pk, o + 3, ptr[s], o + 3, s, n, m, cut);
      std::vector<uint8_t> bad = pk;
      const uint32_t all = 0xffffffffu;
      memcpy(&bad[o], &all, 4);
      refused_pols(bad, ptr[s + 1], ptr[s], ptr[s + 1], s, n, m, cut);
      o += 4;
      for (uint32_t e = 0; e < kk; e++, o += 36) {
        if (e) refused_pols(pk, o, ptr[s], o, s, n, m, cut);
        refused_pols(pk, o + 35, ptr[s], o + 35, s, n, m, cut);
        bad = pk;
        memcpy(&bad[o], &m, 4);  // a row at the bound; one below it is a row like any other
        refused_pols(bad, ptr[s + 1], ptr[s], ptr[s + 1], s, n, m, fmt("constraint index %u >= domainSize %u", m, m));
        const uint32_t last = m - 1;
        memcpy(&bad[o], &last, 4);
        Exact ex(bad, ptr[s + 1]);
        KeyRows ok;
        CHECK(pols_to_rows(ex.p, ptr[s], ptr[s + 1], s, n, m, ok) == 0 && ok.rowptr[m] == now[s].rowptr[m]);
      }
    }
    CHECK(o == ptr[s + 1]);
    std::vector<uint8_t> bad(pk.begin(), pk.begin() + ptr[s + 1]);
    for (size_t extra = 1; extra <= 40; extra += 3) {  // bytes after the last signal's list, whatever they would parse as
      bad.resize(ptr[s + 1] + extra, 0);
      refused_pols(bad, bad.size(), ptr[s], bad.size(), s, n, m, fmt("pols section %d has trailing bytes", s));
    }
  }
}

int main() {
  for (unsigned k = 0; k < 27; k++) {
    CHECK(domain_log2(1u << k) == k);
    if (k) CHECK(domain_log2((1u << k) + 1) == k + 1 && domain_log2((1u << k) - 1) == (k == 1 ? 0 : k));
  }
  for (unsigned bits = 0; bits <= 26; bits += 13)
    for (int i = 0; i < 64; i++) {
      const uint32_t x = (uint32_t)(rnd() & ((1ull << bits) - 1));
      uint32_t r = 0;
      for (uint32_t b = 0; b < bits; b++) r |= ((x >> b) & 1) << (bits - 1 - b);  // the loader's own loop
      CHECK(bitrev32(x, bits) == r && bitrev32(r, bits) == x);
    }
  for (unsigned wild = 0; wild < 4; wild++) {
    run(1, 0, 1, wild);    // domain 2
    run(2, 1, 1, wild);    // p + 1 = n
    run(6, 2, 5, wild);    // nC + p + 1 = 8 exactly
    run(6, 2, 6, wild);    // one more: domain 16
    run(12, 11, 4, wild);  // every signal public, nC + p + 1 = 16
    run(40, 3, 29, wild);
  }
  if (fails) { fprintf(stderr, "qap_forms_selfcheck: %d check(s) failed\n", fails); return 1; }
  printf("qap_forms_selfcheck: ok (%d refusals)\n", refusals);
  return 0;
}
