// websnark_writer.hpp -- the byte layout binarifyProvingKey writes (binarify.ts:143-206), as arithmetic and as a writer, host only:
//   n p m | seven u32 offsets | alfa1 beta1 delta1 beta2 delta2 (448 B) | polsA | polsB | A | B1 | B2 | C | hExps
// pols: per signal a u32 count, then (u32 constraint index, 32 B coefficient) pairs.  The writer takes the two QAP sides as the
// arena holds them -- CSR by row -- and turns them into per-signal lists in one counting pass.  zkr_key_export.hip puts the point
// sections where the plan says; zkr_websnark_render_host (include/zkr.h) copies them from the caller's buffers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkr {

struct WebsnarkPlan {
  uint64_t len = 0;
  uint32_t ptr[7] = {0, 0, 0, 0, 0, 0, 0};  // polsA polsB A B1 B2 C hExps, as the header holds them
  uint64_t count[5] = {0, 0, 0, 0, 0};      // points per section: n n n n-p-1 m
};
constexpr size_t WEBSNARK_POINT_BYTES[5] = {64, 64, 128, 64, 64};

// 0 and the plan, or ZKR_ERR_ARG with a message: sizes that are no key's, or a key past the format's u32 offsets
int websnark_plan(uint64_t n, uint64_t p, uint64_t m, uint64_t nnz_a, uint64_t nnz_b, WebsnarkPlan &pl);

// Header and both pols sections into o[0, pl.ptr[2]).  rowptr[s]: m + 1 entries ascending from 0 to that side's term count (the
// one the plan was made with); col: signal per term; coef: 32 B per term, written as they are.  A signal's list comes out by row
// ascending, terms of one row in their CSR order; nothing is merged or dropped.  ZKR_ERR_ARG: row pointers that do not ascend to
// the plan's term count, or a signal >= n.
int websnark_write_front(uint8_t *o, const WebsnarkPlan &pl, uint32_t n, uint32_t p, uint32_t m, const uint8_t *consts448, const uint32_t *const rowptr[2],
                         const uint32_t *const col[2], const uint8_t *const coef[2]);

}  // namespace zkr
