// The dropout hash shared by every kernel that drops (misc.hip: dropout, the LayerNorm kernels
// that fuse the residual branch's dropout; dwconv7.hip: stochastic depth by sample).
// keep(element i) = hash(seed, i) >= p * 2^32; the per-step part of a device seed (graph replay)
// is mixed in from seed_dev.  Identical masks everywhere: same element index, same hash.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipipe {

__device__ __forceinline__ uint32_t drop_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t drop_base(uint32_t seed, const uint32_t* seed_dev) {
  if (seed_dev != nullptr) {  // L2-served agent-scope load (see attention.hip eff_seed)
    const uint32_t c = __hip_atomic_load(seed_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    seed = drop_mix(seed ^ (c * 0x9e3779b1u + 0x632be5abu));
  }
  return drop_mix(seed * 0x9e3779b1u + 0x7f4a7c15u);
}

__device__ __forceinline__ bool drop_keep(uint32_t base, long idx, uint32_t thr) {
  return drop_mix(base ^ (uint32_t)idx * 0x85ebca77u) >= thr;
}

}  // namespace mipipe
