// layout_selfcheck.cpp -- a stand-alone program over the host shim's plan and layout entry points (msm_plan.hpp), meant for a
// sanitizer build (`make layout-asan`: AddressSanitizer + UBSan on this file and host_arith_shim.cpp, no Python in the process).
// It walks the key shapes of tests/test_proof_layout_cpu.py and a sweep of windows and checks what must hold for ANY shape: every
// table with points lands in exactly one chain and set that exist, a chain's members point back at it, a plan's sizes fit together.
#include <stdint.h>
#include <stdio.h>
#include <stddef.h>

extern "C" {
void zkt_msm_plan(size_t n_scalars, size_t n_points, int c_fixed, uint32_t out[10]);
int zkt_proof_layout(uint32_t n, uint32_t m, const uint32_t npts[5], const uint32_t win_c[5], int share_b, int share_ac, int out[63]);
}

static int fails = 0;
#define CHECK(x) do { if (!(x)) { fails++; fprintf(stderr, "line %d: %s\n", __LINE__, #x); } } while (0)

static void check_plan(size_t ns, size_t np, int c_fixed) {
  uint32_t p[10];  // c, K, glog, nbw, nb, big_thresh, nR, nbl, J, S
  zkt_msm_plan(ns, np, c_fixed, p);
  CHECK(p[0] >= 2 && p[0] <= 22 && (c_fixed == 0 || p[0] == (uint32_t)c_fixed));
  CHECK(p[1] == (255 + p[0] - 1) / p[0] && p[3] == 1u << (p[0] - 1) && p[4] == p[3]);
  CHECK(p[2] <= p[0] - 1 && p[5] >= 64);
  CHECK(p[6] * p[7] == p[3] && p[6] <= 256 && p[8] >= 1 && p[8] <= 64);
  CHECK(p[9] >= 1 && p[9] * (p[0] - 1 - p[2] + 2) <= 256);  // ntask * S <= MSM_THREADS (msm_reduce3_kernel)
}

static void check_layout(uint32_t n, uint32_t m, const uint32_t (&npts)[5], int share_b, int share_ac, const uint32_t (&win)[5], int want_chains) {
  int o[63];
  zkt_proof_layout(n, m, npts, win, share_b, share_ac, o);
  const int n_chains = o[2];
  CHECK(n_chains == want_chains && n_chains >= 0 && n_chains <= 5);
  int members_seen = 0;
  for (int t = 0; t < 5; t++) {
    const int *tb = o + 3 + 5 * t;  // sort_src, chain, set, flags, own_result
    CHECK(tb[0] >= 0 && tb[0] < 5 && (tb[0] == t || npts[tb[0]] == npts[t]));
    CHECK((tb[1] >= 0) == (npts[t] != 0) && tb[1] < n_chains);
    if (tb[1] < 0) { CHECK(!tb[4]); continue; }
    const int *ch = o + 28 + 7 * tb[1];  // n_members, members[2], sets, geom, g2, latency
    CHECK(ch[0] >= 1 && ch[0] <= 2 && (ch[1] == t || ch[2] == t));
    CHECK(tb[2] >= 0 && tb[2] < ch[3] && ch[5] == (t == 2));
    CHECK(tb[4] == (tb[3] != 1));
    members_seen++;
  }
  int members = 0;
  for (int c = 0; c < n_chains; c++) {
    const int *ch = o + 28 + 7 * c;
    members += ch[0];
    CHECK(ch[4] == ch[1] || ch[4] == ch[2]);
  }
  CHECK(members == members_seen);
}

int main() {
  const size_t sizes[][2] = {{1, 1}, {5, 1}, {100, 73}, {1u << 12, 1u << 12}, {1u << 12, 1}, {1u << 17, 87000}, {1u << 20, 1013000}, {1u << 24, 1u << 24}};
  for (const auto &s : sizes) {
    check_plan(s[0], s[1], 0);
    for (int c = 2; c <= 22; c++) check_plan(s[0], s[1], c);
  }
  const uint32_t own[5] = {0, 0, 0, 0, 0};
  check_layout(3000, 4096, {2950, 1500, 1500, 2950, 4096}, 1, 1, own, 3);   // one window: {B2}, {B1, A}, {C, H}
  check_layout(3000, 4096, {2950, 1500, 1400, 2900, 4096}, 1, 1, own, 3);
  check_layout(1500, 4096, {1491, 750, 750, 1491, 4096}, 1, 1, own, 4);     // C's window is not H's
  check_layout(100, 256, {91, 50, 50, 91, 256}, 1, 0, own, 4);
  check_layout(500, 512, {400, 0, 0, 0, 512}, 1, 1, own, 2);                // a shard: A without B
  check_layout(500, 512, {400, 0, 0, 400, 512}, 1, 1, own, 2);
  check_layout(3000, 4096, {2950, 1500, 1500, 0, 4096}, 1, 1, own, 3);      // no C point: H alone
  check_layout(3000, 4096, {2950, 1500, 1500, 2950, 0}, 1, 1, own, 3);
  check_layout(3000, 4096, {0, 0, 0, 0, 0}, 1, 1, own, 0);                  // nothing to multiply
  check_layout(1u << 20, 1u << 20, {1013000, 700000, 700000, 1013000, 1u << 20}, 1, 1, {20, 20, 20, 20, 20}, 3);
  check_layout(4096, 4096, {4000, 2000, 2000, 4000, 4096}, 1, 1, {12, 12, 12, 12, 11}, 4);
  printf(fails ? "layout selfcheck: %d FAILED\n" : "layout selfcheck ok\n", fails);
  return fails ? 1 : 0;
}
