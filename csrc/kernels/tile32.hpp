// mfma_f32_32x32x16_bf16 in "swapped" orientation (a lane owns a column of the result), as the
// attention kernels use it (attention.hip, and the window kernels through wintile.hpp): the
// product, its accumulator's register <-> row map, and an accumulator packed as the next
// product's B operand.
#pragma once
#include "common.hpp"

namespace mipipe {
namespace tile32 {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short s16x8;

__device__ __forceinline__ f32x16 mfma32(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
// reg i of a 32x32 accumulator <-> row (i&3) + 8(i>>2) + 4h (h = lane >> 5), column lane & 31
__device__ __forceinline__ int acc_row(int i, int hl) { return (i & 3) + 8 * (i >> 2) + 4 * hl; }
// regs 8s..8s+7 of an accumulator as the B operand of the next product (k = its rows)
__device__ __forceinline__ bf16x8 pack_acc(const f32x16& x, int s) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (__bf16)x[8 * s + j];
  return v;
}

}  // namespace tile32
}  // namespace mipipe
