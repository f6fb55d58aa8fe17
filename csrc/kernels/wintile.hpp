// The 64-token x 32-wide tile pieces the window-attention kernels share (winattn.hip: 7x7
// windows, winattn8.hip: 8x8 windows with cosine scores): the 32x32x16 bf16 MFMA in "swapped"
// orientation (a lane owns a column, so a softmax row is in-lane), an accumulator packed as the
// next product's B operand, [64][32] bf16 LDS images and their transposed reads.
#pragma once
#include "common.hpp"

namespace mipipe {
namespace wintile {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) short s16x8;

constexpr int kPitch = 80;            // bytes per row of a [64][32] bf16 LDS image (16-B aligned)
constexpr int kImg = 64 * kPitch;

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
// A operand holding Tᵀ of a row-major [64][32] image T, k (row) order of pack_acc: element j of
// lane half h <-> row r0 + 8(j>>2) + 4h + (j&3); the lane's column is lane & 31.
__device__ __forceinline__ bf16x8 ld_tr(const char* img, uint32_t r0, int lane) {
  const uint32_t hl = lane >> 5, li = lane & 15, q = li >> 2, p = li & 3;
  const char* a0 = img + (r0 + 4 * hl + q) * kPitch + (16 * ((lane >> 4) & 1) + 4 * p) * 2;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(a0 + 8 * kPitch));
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
// this wave's LDS accesses so far have completed; nothing moves across (wave-private images)
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// the lane's operand fragments (row = 32t + (lane & 31), elements 16st + 8hl ..) -> the image
__device__ __forceinline__ void st_image(char* img, const bf16x8 (&f)[2][2], int lane) {
  const int r = lane & 31, hl = lane >> 5;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int st = 0; st < 2; ++st)
      *reinterpret_cast<bf16x8*>(img + (32 * t + r) * kPitch + (16 * st + 8 * hl) * 2) = f[t][st];
}
// accumulator (lane = token column, regs = d rows) -> 8-byte pieces of the token's head slice
__device__ __forceinline__ void st_cols(__bf16* dst, const f32x16& x, float s, int hl) {
#pragma unroll
  for (int ig = 0; ig < 4; ++ig)
    *reinterpret_cast<uint2*>(dst + 8 * ig + 4 * hl) =
        make_uint2(pack2(x[4 * ig] * s, x[4 * ig + 1] * s),
                   pack2(x[4 * ig + 2] * s, x[4 * ig + 3] * s));
}

}  // namespace wintile
}  // namespace mipipe
