// zkr_selftest.hip -- the group law of curve29.hpp as the DEVICE compiles it (every product one opaque asm statement, a scheduling
// barrier between products, the special cases as per-lane branches), on raw limbs: zkr_selftest_curve29.  One thread per record
// runs curve29_raw_op (curve29_raw.hpp), the function the host shim runs on the same records; tests/test_gpu_group_law.py compares
// the two limb for limb and both with integer arithmetic.  Beside it the 8 x 32-bit-limb field of field.hpp -- the product
// scanning in the 96-bit column accumulator, the fused sums of field_fused.hpp, the schoolbook Fq2 product and both mul_sub, none of
// which the host build shares -- the same way: zkr_selftest_fp runs field_raw_op (field_raw.hpp) and tests/test_gpu_field_raw.py
// compares.  A translation unit of its own: test hooks only, no kernel of the proving path is in it or changed by it.
#include "zkr_internal.hpp"
#include "curve29_raw.hpp"
#include "field_raw.hpp"

namespace zkr {

// 128 threads per workgroup, and said so: with the default bound (1024) the compiler keeps a kernel to 128 VGPRs and the G2 forms,
// which the proving path runs in up to 248, would spill
template <class C, int OP>
static __global__ void __launch_bounds__(128) curve29_raw_kernel(const uint32_t *in, size_t n, uint32_t *out, uint8_t *inf) {
  constexpr int RW = curve29_record_words(Raw29<C>::g2, OP), OW = curve29_out_words(Raw29<C>::g2, OP);
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  curve29_raw_op<C, OP>(in + i * RW, out + i * OW, inf + i);
}

template <class C, int OP>
static void curve29_raw_launch(const uint32_t *d_in, size_t n, uint32_t *d_out, uint8_t *d_inf) {
  curve29_raw_kernel<C, OP><<<(unsigned)((n + 127) / 128), 128>>>(d_in, n, d_out, d_inf);
}
template <class C>
static void curve29_raw_dispatch(int op, const uint32_t *d_in, size_t n, uint32_t *d_out, uint8_t *d_inf) {
  switch (op) {
    case 0: curve29_raw_launch<C, 0>(d_in, n, d_out, d_inf); break;
    case 1: curve29_raw_launch<C, 1>(d_in, n, d_out, d_inf); break;
    case 2: curve29_raw_launch<C, 2>(d_in, n, d_out, d_inf); break;
    case 3: curve29_raw_launch<C, 3>(d_in, n, d_out, d_inf); break;
    case 4: curve29_raw_launch<C, 4>(d_in, n, d_out, d_inf); break;
    case 5: curve29_raw_launch<C, 5>(d_in, n, d_out, d_inf); break;
    default: curve29_raw_launch<C, 6>(d_in, n, d_out, d_inf);
  }
}

// one thread per record, as above; 128 threads per workgroup leave the Fq2 forms (eight operands live, two fused sums) their registers
template <class PM, int OP>
static __global__ void __launch_bounds__(128) field_raw_kernel(const uint32_t *in, size_t n, uint32_t *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  field_raw_op<PM, OP>(in + i * FIELD_RAW_RECORD_WORDS, out + i * field_raw_out_words(OP));
}
template <class PM>
static void field_raw_launch(int op, const uint32_t *d_in, size_t n, uint32_t *d_out) {
  field_raw_dispatch<PM>(op, [&](auto tag) { field_raw_kernel<PM, decltype(tag)::value><<<(unsigned)((n + 127) / 128), 128>>>(d_in, n, d_out); });
}

}  // namespace zkr

using namespace zkr;

extern "C" int zkr_selftest_curve29(int device, int g2, int op, const uint32_t *records, size_t n, uint32_t *out, uint8_t *inf) {
  if (!records || !out || !inf || op < 0 || op >= CURVE29_OPS || (g2 != 0 && g2 != 1)) { set_error("bad argument"); return ZKR_ERR_ARG; }
  if (n > ((size_t)1 << 24)) { set_error("too many records for the group-law self test"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  if (n == 0) return 0;
  ZKR_HIP_CHECK(hipSetDevice(device));
  const size_t in_bytes = n * (size_t)curve29_record_words(g2 != 0, op) * 4, out_bytes = n * (size_t)curve29_out_words(g2 != 0, op) * 4;
  DevBuf d_in, d_out, d_inf;
  int rc;
  if ((rc = d_in.alloc(in_bytes)) || (rc = d_out.alloc(out_bytes)) || (rc = d_inf.alloc(n))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(d_in.p, records, in_bytes, hipMemcpyHostToDevice));
  if (g2) curve29_raw_dispatch<G2C>(op, d_in.as<uint32_t>(), n, d_out.as<uint32_t>(), d_inf.as<uint8_t>());
  else curve29_raw_dispatch<G1C>(op, d_in.as<uint32_t>(), n, d_out.as<uint32_t>(), d_inf.as<uint8_t>());
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
  ZKR_HIP_CHECK(hipMemcpy(inf, d_inf.p, n, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int zkr_selftest_fp(int device, int field, int op, const uint32_t *records, size_t n, uint32_t *out) {
  if (!records || !out || !field_raw_valid(field, op)) { set_error("bad argument"); return ZKR_ERR_ARG; }
  if (n > ((size_t)1 << 24)) { set_error("too many records for the field self test"); return ZKR_ERR_ARG; }
  if (int rc = need_device(device)) return rc;
  if (n == 0) return 0;
  ZKR_HIP_CHECK(hipSetDevice(device));
  const size_t in_bytes = n * (size_t)FIELD_RAW_RECORD_WORDS * 4, out_bytes = n * (size_t)field_raw_out_words(op) * 4;
  DevBuf d_in, d_out;
  int rc;
  if ((rc = d_in.alloc(in_bytes)) || (rc = d_out.alloc(out_bytes))) return rc;
  ZKR_HIP_CHECK(hipMemcpy(d_in.p, records, in_bytes, hipMemcpyHostToDevice));
  if (field) field_raw_launch<FrParams>(op, d_in.as<uint32_t>(), n, d_out.as<uint32_t>());
  else field_raw_launch<FqParams>(op, d_in.as<uint32_t>(), n, d_out.as<uint32_t>());
  ZKR_HIP_CHECK(hipGetLastError());
  ZKR_HIP_CHECK(hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
  return 0;
}
