// key_export_selfcheck.cpp -- a stand-alone program over zkr_websnark_len and zkr_websnark_render_host (websnark_writer.cpp: the
// arithmetic and the writer of the websnark proving-key layout, which zkr_key_export_websnark renders a device key with), meant
// for a sanitizer build (`make key-export-asan`: AddressSanitizer + UBSan on this file and websnark_writer.cpp, no Python and no
// HIP in the process).  It renders generated keys from exactly-sized heap arrays -- rows of every width, empty rows, empty
// signals, one (signal, row) stored twice, zero coefficients -- reads the bytes back with a reader of its own and checks what must
// hold for ANY input: the length is the planned one, the offsets tile the buffer, every signal's list ascends by row and keeps the
// stored order inside a row, no term is lost, merged or invented, the point sections are the caller's.  Then the refusals.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/zkr.h"

namespace zkr {
void set_error(const char *fmt, ...) {  // the library's lives beside its HIP code
  va_list ap;
  va_start(ap, fmt);
  va_end(ap);
}
}  // namespace zkr
extern "C" void zkr_free(void *p) { free(p); }  // as the library's (zkr_key.hip)

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fails++; fprintf(stderr, "line %d: %s\n", __LINE__, #x); } } while (0)

static uint64_t rng_state = 0x5A4B0001;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// an array of exactly `count` elements on the heap: a read or write one past it is the sanitizer's to find
template <class T>
struct Exact {
  T *p;
  size_t count;
  explicit Exact(size_t n) : p((T *)malloc(n ? n * sizeof(T) : 1)), count(n) {}
  ~Exact() { free(p); }
  Exact(const Exact &) = delete;
};

struct Term { uint32_t row, sig; uint8_t coef[32]; };

static void run(uint32_t n, uint32_t p, uint32_t m, unsigned max_width, unsigned wild) {
  const size_t pcount[5] = {n, n, n, n - p - 1, m}, pbytes[5] = {64, 64, 128, 64, 64};
  std::vector<Term> side[2];
  for (int s = 0; s < 2; s++)
    for (uint32_t r = 0; r < m; r++) {
      unsigned w = (unsigned)(rnd() % (max_width + 1));
      if (rnd() % 4 == 0) w = 0;
      for (unsigned k = 0; k < w; k++) {
        Term t;
        t.row = r;
        t.sig = (wild & 1) && k ? side[s].back().sig : (uint32_t)(rnd() % n);  // wild 1: one (signal, row) many times over
        if ((wild & 2) && rnd() % 3 == 0) t.sig = 0;                           // wild 2: a long list for signal 0
        for (int b = 0; b < 32; b += 8) { uint64_t v = rnd() % 5 == 0 ? 0 : rnd(); memcpy(t.coef + b, &v, 8); }
        if (rnd() % 7 == 0) memset(t.coef, 0, 32);
        side[s].push_back(t);
      }
    }
  Exact<uint32_t> rowptr0(m + 1), rowptr1(m + 1), col0(side[0].size()), col1(side[1].size());
  Exact<uint8_t> coef0(side[0].size() * 32), coef1(side[1].size() * 32), consts(448);
  Exact<uint32_t> *rowptr[2] = {&rowptr0, &rowptr1}, *col[2] = {&col0, &col1};
  Exact<uint8_t> *coef[2] = {&coef0, &coef1};
  for (int s = 0; s < 2; s++) {
    size_t e = 0;
    for (uint32_t r = 0; r <= m; r++) {
      while (e < side[s].size() && side[s][e].row < r) e++;
      rowptr[s]->p[r] = (uint32_t)e;
    }
    for (e = 0; e < side[s].size(); e++) { col[s]->p[e] = side[s][e].sig; memcpy(coef[s]->p + e * 32, side[s][e].coef, 32); }
  }
  for (int i = 0; i < 448; i++) consts.p[i] = (uint8_t)rnd();
  Exact<uint8_t> pt0(pcount[0] * pbytes[0]), pt1(pcount[1] * pbytes[1]), pt2(pcount[2] * pbytes[2]), pt3(pcount[3] * pbytes[3]), pt4(pcount[4] * pbytes[4]);
  Exact<uint8_t> *pts[5] = {&pt0, &pt1, &pt2, &pt3, &pt4};
  const uint8_t *points[5];
  for (int t = 0; t < 5; t++) {
    for (size_t i = 0; i < pts[t]->count; i++) pts[t]->p[i] = (uint8_t)rnd();
    points[t] = pts[t]->p;
  }

  uint64_t want_len = 0;
  CHECK(zkr_websnark_len(n, p, m, side[0].size(), side[1].size(), &want_len) == 0);
  void *out = nullptr;
  size_t len = 0;
  int rc = zkr_websnark_render_host(n, p, m, consts.p, rowptr0.p, col0.p, coef0.p, rowptr1.p, col1.p, coef1.p, points, &out, &len);
  CHECK(rc == 0 && out && len == want_len);
  if (rc || !out) return;
  // the same bytes in a block of exactly that length: every read below stays inside what the writer said it wrote
  Exact<uint8_t> pk(len);
  memcpy(pk.p, out, len);
  zkr_free(out);
  const uint8_t *b = pk.p;
  CHECK(rd32(b) == n && rd32(b + 4) == p && rd32(b + 8) == m);
  uint32_t ptr[7];
  for (int i = 0; i < 7; i++) ptr[i] = rd32(b + 12 + 4 * i);
  CHECK(ptr[0] == 488 && memcmp(b + 40, consts.p, 448) == 0);
  for (int s = 0; s < 2; s++) {
    // read the lists back into rows: signals ascending, which is the stored order of a row sorted stably by signal
    std::vector<Term> back;
    size_t o = ptr[s];
    for (uint32_t sig = 0; sig < n && o + 4 <= ptr[s + 1]; sig++) {
      const uint32_t k = rd32(b + o);
      o += 4;
      CHECK(o + 36ull * k <= ptr[s + 1]);
      if (o + 36ull * k > ptr[s + 1]) break;
      uint32_t last = 0;
      for (uint32_t e = 0; e < k; e++, o += 36) {
        Term t;
        t.row = rd32(b + o);
        t.sig = sig;
        memcpy(t.coef, b + o + 4, 32);
        CHECK(t.row < m && (e == 0 || t.row >= last));
        last = t.row;
        back.push_back(t);
      }
    }
    CHECK(o == ptr[s + 1]);
    CHECK(back.size() == side[s].size());
    auto by_row_sig = [](const Term &x, const Term &y) { return x.row != y.row ? x.row < y.row : x.sig < y.sig; };
    std::vector<Term> want = side[s];
    std::stable_sort(want.begin(), want.end(), by_row_sig);
    std::stable_sort(back.begin(), back.end(), by_row_sig);
    bool same = want.size() == back.size();
    for (size_t e = 0; same && e < want.size(); e++) same = want[e].row == back[e].row && want[e].sig == back[e].sig && !memcmp(want[e].coef, back[e].coef, 32);
    CHECK(same);
  }
  size_t o = ptr[2];
  for (int t = 0; t < 5; t++) {
    CHECK(ptr[2 + t] == o);
    CHECK(o + pts[t]->count <= len && (pts[t]->count == 0 || memcmp(b + o, pts[t]->p, pts[t]->count) == 0));
    o += pts[t]->count;
  }
  CHECK(o == len);

  // refusals leave nothing behind and read nothing past the arrays
  if (!side[0].empty()) {
    void *none = nullptr;
    size_t none_len = 0;
    const uint32_t keep = col0.p[0];
    col0.p[0] = n;
    CHECK(zkr_websnark_render_host(n, p, m, consts.p, rowptr0.p, col0.p, coef0.p, rowptr1.p, col1.p, coef1.p, points, &none, &none_len) == ZKR_ERR_ARG && !none);
    col0.p[0] = keep;
    uint32_t r = 0;
    while (rowptr0.p[r + 1] == rowptr0.p[r]) r++;
    if (r > 0) {
      const uint32_t keep_r = rowptr0.p[r];
      rowptr0.p[r] = rowptr0.p[r + 1] + 1;  // above its successor
      CHECK(zkr_websnark_render_host(n, p, m, consts.p, rowptr0.p, col0.p, coef0.p, rowptr1.p, col1.p, coef1.p, points, &none, &none_len) == ZKR_ERR_ARG && !none);
      rowptr0.p[r] = keep_r;
    }
    rowptr0.p[0] = 1;
    CHECK(zkr_websnark_render_host(n, p, m, consts.p, rowptr0.p, col0.p, coef0.p, rowptr1.p, col1.p, coef1.p, points, &none, &none_len) == ZKR_ERR_ARG && !none);
    rowptr0.p[0] = 0;
  }
}

int main() {
  for (unsigned wild = 0; wild < 4; wild++) {
    run(1, 0, 2, 3, wild);
    run(2, 1, 2, 1, wild);
    run(5, 0, 4, 0, wild);  // no term at all
    run(37, 7, 64, 4, wild);
    run(128, 7, 128, 12, wild);  // rows wider than the prover's wide-row threshold
    run(300, 299, 256, 3, wild);  // every signal public: an empty C section
  }
  uint64_t len = 0;
  CHECK(zkr_websnark_len(4, 1, 4, 3, 2, &len) == 0 && len == 488 + 2 * 16 + 36 * 5 + 64 * 4 * 2 + 128 * 4 + 64 * 2 + 64 * 4);
  CHECK(zkr_websnark_len(4, 1, 4, 3, 2, nullptr) == ZKR_ERR_ARG);
  CHECK(zkr_websnark_len(0, 0, 4, 0, 0, &len) == ZKR_ERR_ARG && zkr_websnark_len(4, 4, 4, 0, 0, &len) == ZKR_ERR_ARG && zkr_websnark_len(4, 1, 6, 0, 0, &len) == ZKR_ERR_ARG);
  CHECK(zkr_websnark_len(1ull << 23, 73, 1ull << 23, 2ull << 23, 2ull << 23, &len) == ZKR_ERR_ARG);  // 4.5 GB: past the u32 offsets
  CHECK(zkr_websnark_len(1ull << 22, 73, 1ull << 22, 2ull << 22, 2ull << 22, &len) == 0 && len > (1ull << 31));
  CHECK(zkr_websnark_len(~0ull, 1, 1ull << 20, ~0ull, ~0ull, &len) == ZKR_ERR_ARG);  // nothing wraps
  if (fails) { fprintf(stderr, "key_export_selfcheck: %d check(s) failed\n", fails); return 1; }
  printf("key_export_selfcheck: ok\n");
  return 0;
}
