// The one access layer of the kernels that stream over the flat fp32 parameter buffer: the
// optimizers (optim.hip) and the weight EMA (ema.hip).  The rules that keep these kernels at
// memory speed live here, as code:
//
//   streaming state   p, g, m, v and the EMA are 16 B per parameter each and touched once per pass:
//                     with bit 1024 of g_nt_store set they are read and written non-temporally
//                     (ld4 / st4 with NT), so a pass does not evict what the next kernels need.
//   cached shadow     the bf16 copy of the weights is what the next forward reads: st_shadow is
//                     always a plain store.
//   loads before uses every load of a round (chunk walk) or of a tile (tile walk) is issued before
//                     the first value is used: U x NA x 16 B of each thread in flight.
//   no load behind a branch
//                     the compiler closes a conditional load with a full vmcnt(0) drain, or sinks
//                     the load into the branch.  A lane past the end therefore re-reads the last
//                     valid item (chunk walk) or runs in the guarded loop of the one partial tile
//                     (tile walk); only uses and stores are conditional.
#pragma once
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

typedef __attribute__((ext_vector_type(4))) float f4v;

// float4 item i of a flat fp32 array
template <bool NT>
__device__ __forceinline__ float4 ld4(const float* p, long i) {
  if constexpr (NT) {
    const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p) + i);
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return reinterpret_cast<const float4*>(p)[i];
  }
}
template <bool NT>
__device__ __forceinline__ void st4(float* p, long i, const float (&a)[4]) {
  if constexpr (NT) {
    __builtin_nontemporal_store(f4v{a[0], a[1], a[2], a[3]}, reinterpret_cast<f4v*>(p) + i);
  } else {
    reinterpret_cast<float4*>(p)[i] = make_float4(a[0], a[1], a[2], a[3]);
  }
}
__device__ __forceinline__ void unpack(const float4& v, float (&a)[4]) {
  a[0] = v.x;
  a[1] = v.y;
  a[2] = v.z;
  a[3] = v.w;
}
// bf16 shadow of item i (sh may be null: no shadow); see "cached shadow" above
__device__ __forceinline__ void st_shadow(__bf16* sh, long i, const float* a) {
  if (sh != nullptr) reinterpret_cast<uint2*>(sh)[i] = pack4(a);
}

// ---- chunk walk: one block per chunk of an optimizer's chunk table --------------------------
// A chunk entry {segment, offset / 64, length, 0} the kernels may act on: inside the buffer,
// 64-aligned, of a known segment.  The host builds the table from FlatParamSpace.ranges(); a
// block given anything else does nothing.  Every kernel starts with
//   const int4 c = chunks[blockIdx.x];  if (!chunk_ok(c, n, nseg)) return;
// and may then index the segment table with c.x.
__device__ __forceinline__ bool chunk_ok(const int4& c, long n, int nseg) {
  return c.x >= 0 && c.x < nseg && c.y >= 0 && c.z > 0 && c.z <= kOptimChunk && (c.z & 63) == 0 &&
         (long)c.y * 64 + c.z <= n;
}

// 256 threads walk the checked chunk c in rounds of U x 256 items.  Per round U items of each of
// the NA arrays are loaded (clamped to the chunk's last item), then body(item, x) runs once per
// item inside the chunk: x[a] is the item's float4 of src[a].  A round ends at the first item
// past the chunk's end.  A body whose bits matter writes its fmas out (lamb_moments_kernel): which
// product of a b + c d the compiler fuses depends on the code around the expression.
// seg_sumsq_kernel keeps this loop written out, for the reason given there.
constexpr int kChunkRounds = kOptimChunk / 4 / 256;  // float4 items per thread of a full chunk
static_assert(kOptimChunk % 1024 == 0, "a chunk is a whole number of 256-thread float4 rounds");
template <bool NT, int U, int NA, class Body>
__device__ __forceinline__ void chunk_walk(const int4& c, const float* const (&src)[NA],
                                           Body&& body) {
  const long base = (long)c.y * 16;
  const int len4 = c.z >> 2;
  for (int r = 0; r < kChunkRounds && r * 256 < len4; r += U) {
    float4 v[U][NA];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = base + min((r + u) * 256 + (int)threadIdx.x, len4 - 1);
#pragma unroll
      for (int a = 0; a < NA; ++a) v[u][a] = ld4<NT>(src[a], j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = (r + u) * 256 + threadIdx.x;
      if (i >= len4) break;
      body(base + i, v[u]);
    }
  }
}

// ---- tile walk: block b owns float4 items [b * TILE4, (b + 1) * TILE4) of n4 ----------------
// TILE4 / 256 items per thread.  Every block but the last has a whole tile and runs without a
// per-lane condition; only the buffer's last, partial tile runs the guarded loop.
// body(item, x) as above.
template <bool NT, int TILE4, int NA, class Body>
__device__ __forceinline__ void tile_walk(long n4, const float* const (&src)[NA], Body&& body) {
  constexpr int U = TILE4 / 256;
  const long base = (long)blockIdx.x * TILE4 + threadIdx.x;
  if ((long)(blockIdx.x + 1) * TILE4 <= n4) {
    float4 v[U][NA];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int a = 0; a < NA; ++a) v[u][a] = ld4<NT>(src[a], base + u * 256);
#pragma unroll
    for (int u = 0; u < U; ++u) body(base + u * 256, v[u]);
    return;
  }
  for (long i = base; i < n4; i += 256) {
    float4 x[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) x[a] = ld4<NT>(src[a], i);
    body(i, x);
  }
}

// ---- host side: the streaming bit into a template argument -----------------------------------
inline bool flat_nt() { return (g_nt_store & 1024) != 0; }  // the one reader of the streaming bit

template <class F>
inline void dispatch_nt(F&& f) {
  dispatch_bool(flat_nt(), f);  // common.hpp
}

}  // namespace mipipe
