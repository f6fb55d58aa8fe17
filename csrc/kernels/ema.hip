// Exponential moving average of the model weights over the flat fp32 parameter buffer, and the
// in-place exchange that puts the averaged weights under the model (mipipe/optim/ema.py).
//
//   ema_update   e = e + w (p - e) over the flat buffer, every `every`-th call
//   ema_swap     p' = e, e' = p, shadow' = bf16(p'): a pure exchange, so two swaps restore all
//                three buffers bit for bit
//   ema_buffers_update / ema_buffers_swap
//                the same two operations for the module's fp32 buffers (BatchNorm running
//                statistics): many small tensors outside the flat space, reached through a
//                device table of rows {address, offset into the EMA's own flat copy, length}
//
// No host value enters a launch.  The number of update() calls lives on the device (t_dev, advanced
// by a device op before the launch) and every block derives from it whether this call averages at
// all and with which weight, so an update captured into a hipGraph replays correctly:
//
//   t % every != 0:  the block returns without touching memory
//   u = t / every - 1                                   index of this averaging update, from 0
//   w = warmup ? max(w_min, 9 / (10 + u)) : w_min       w_min = float32(1 - decay), from the host
//
// 9 / (10 + u) is 1 - (1 + u) / (10 + u), timm's warm-up decay, without the cancellation of the
// subtraction.  e + w (p - e) is a rounded subtract, a rounded multiply and a rounded add
// (contraction off, as in batch_mix and lamb_u).  Padding (alignment tails, reserved pad rows) is
// zero in p and e: 0 + w (0 - 0) is exactly 0, and an exchange of zeros leaves zeros.
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

// float4 items per block, measured at the ResNet-50 and BERT-base flat sizes with the buffers not
// in the memory-side cache (profiles/model_ema.txt): streaming accesses are fastest with four
// items of each array in flight per thread and no loop, cached accesses with one (many small
// blocks, as ATen's elementwise kernels have them).  Larger tiles and persistent grids lost 2-7 %.
constexpr int kEmaTileNT = 1024;
constexpr int kEmaTileCached = 256;

// streaming (non-temporal) access, as in optim.hip: the average is touched once per step
typedef __attribute__((ext_vector_type(4))) float f4v;
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
__device__ __forceinline__ void st4(float* p, long i, const float* a) {
  if constexpr (NT) {
    __builtin_nontemporal_store(f4v{a[0], a[1], a[2], a[3]}, reinterpret_cast<f4v*>(p) + i);
  } else {
    reinterpret_cast<float4*>(p)[i] = make_float4(a[0], a[1], a[2], a[3]);
  }
}

// This call's averaging weight from the device call count; false: the call is skipped.
__device__ __forceinline__ bool ema_weight(const int* __restrict__ t_dev, int every, float w_min,
                                           int warmup, float* w) {
  const int t = __hip_atomic_load(t_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (every < 1 || t < every || t % every != 0) return false;
  const int u = t / every - 1;
  *w = warmup ? fmaxf(w_min, __fdiv_rn(9.0f, (float)(10 + u))) : w_min;
  return true;
}

// e + w (p - e) in three roundings (hipcc would contract the multiply and the add into v_fma_f32)
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
#pragma clang fp contract(off)
  const float d = p - e;
  const float q = w * d;
  return e + q;
}

// Block b owns float4 items [b * TILE4, (b + 1) * TILE4) of n4, U = TILE4 / 256 per thread.  Every block but the last
// has a whole tile and runs without a per-lane condition: every item of each array is loaded before
// any is used and no load sits behind a branch (the compiler would close it with a full vmcnt(0)
// drain, or sink the load into the branch).  Only the buffer's last, partial tile is guarded.
template <bool NT, int TILE4>
__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p,
                                                         float* __restrict__ e, long n4,
                                                         const int* __restrict__ t_dev, int every,
                                                         float w_min, int warmup,
                                                         float* __restrict__ scal) {
  float w;
  if (!ema_weight(t_dev, every, w_min, warmup, &w)) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[0] = w;
  constexpr int U = TILE4 / 256;
  const long base = (long)blockIdx.x * TILE4 + threadIdx.x;
  if ((long)(blockIdx.x + 1) * TILE4 <= n4) {
    float4 pv[U], ev[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pv[u] = ld4<NT>(p, base + u * 256);
      ev[u] = ld4<NT>(e, base + u * 256);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float ea[4] = {ema_lerp(ev[u].x, pv[u].x, w), ema_lerp(ev[u].y, pv[u].y, w),
                           ema_lerp(ev[u].z, pv[u].z, w), ema_lerp(ev[u].w, pv[u].w, w)};
      st4<NT>(e, base + u * 256, ea);
    }
    return;
  }
  for (long i = base; i < n4; i += 256) {
    const float4 pv = ld4<NT>(p, i), ev = ld4<NT>(e, i);
    const float ea[4] = {ema_lerp(ev.x, pv.x, w), ema_lerp(ev.y, pv.y, w),
                         ema_lerp(ev.z, pv.z, w), ema_lerp(ev.w, pv.w, w)};
    st4<NT>(e, i, ea);
  }
}

// p and e exchanged; the bf16 shadow of the new p written with the optimizer kernels' conversion
// (cached store: the next forward reads it).
template <bool NT>
__device__ __forceinline__ void ema_swap_store(float* p, float* e, __bf16* sh, long i,
                                               const float4& pv, const float4& ev) {
  const float pa[4] = {pv.x, pv.y, pv.z, pv.w};
  const float ea[4] = {ev.x, ev.y, ev.z, ev.w};
  st4<NT>(p, i, ea);
  st4<NT>(e, i, pa);
  if (sh != nullptr)
    reinterpret_cast<uint2*>(sh)[i] = make_uint2(pack2(ea[0], ea[1]), pack2(ea[2], ea[3]));
}

template <bool NT, int TILE4>
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p,
                                                       float* __restrict__ e,
                                                       __bf16* __restrict__ sh, long n4) {
  constexpr int U = TILE4 / 256;
  const long base = (long)blockIdx.x * TILE4 + threadIdx.x;
  if ((long)(blockIdx.x + 1) * TILE4 <= n4) {
    float4 pv[U], ev[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      pv[u] = ld4<NT>(p, base + u * 256);
      ev[u] = ld4<NT>(e, base + u * 256);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) ema_swap_store<NT>(p, e, sh, base + u * 256, pv[u], ev[u]);
    return;
  }
  for (long i = base; i < n4; i += 256) {
    const float4 pv = ld4<NT>(p, i), ev = ld4<NT>(e, i);
    ema_swap_store<NT>(p, e, sh, i, pv, ev);
  }
}

// A table row the buffer kernels may act on: a 4-byte aligned source, a length within one block's
// reach, a destination inside the EMA's copy.  The host builds the table from the module's
// buffers; a block given anything else does nothing.
struct EmaRow {
  float* src;
  long off;
  int len;
};
__device__ __forceinline__ bool ema_row(const long* __restrict__ table, long nbuf, EmaRow* r) {
  const long* t = table + 3 * (long)blockIdx.x;
  const unsigned long a = (unsigned long)t[0];
  r->src = reinterpret_cast<float*>(a);
  r->off = t[1];
  r->len = (int)t[2];
  return a != 0 && (a & 3) == 0 && t[2] > 0 && t[2] <= kEmaRowMax && t[1] >= 0 &&
         t[1] + t[2] <= nbuf;
}

// One block per row, 4-byte accesses (the sources need not be 16-byte aligned; ~200 KB in all).
__global__ __launch_bounds__(256) void ema_buffers_update_kernel(
    const long* __restrict__ table, float* __restrict__ eb, long nbuf,
    const int* __restrict__ t_dev, int every, float w_min, int warmup) {
  float w;
  if (!ema_weight(t_dev, every, w_min, warmup, &w)) return;
  EmaRow r;
  if (!ema_row(table, nbuf, &r)) return;
  for (int i = threadIdx.x; i < r.len; i += 256)
    eb[r.off + i] = ema_lerp(eb[r.off + i], r.src[i], w);
}

__global__ __launch_bounds__(256) void ema_buffers_swap_kernel(const long* __restrict__ table,
                                                               float* __restrict__ eb,
                                                               long nbuf) {
  EmaRow r;
  if (!ema_row(table, nbuf, &r)) return;
  for (int i = threadIdx.x; i < r.len; i += 256) {
    const float a = r.src[i], b = eb[r.off + i];
    r.src[i] = b;
    eb[r.off + i] = a;
  }
}

inline bool nt_state() { return (g_nt_store & 1024) != 0; }

inline int ema_grid(long n4, int tile4) { return (int)((n4 + tile4 - 1) / tile4); }

}  // namespace

void ema_update(const float* p, float* e, long n, const int* t_dev, int every, float w_min,
                bool warmup, float* scal, hipStream_t st) {
  if (n <= 0) return;
  const long n4 = n / 4;
  if (nt_state())
    hipLaunchKernelGGL((ema_update_kernel<true, kEmaTileNT>), dim3(ema_grid(n4, kEmaTileNT)),
                       dim3(256), 0, st, p, e, n4, t_dev, every, w_min, (int)warmup, scal);
  else
    hipLaunchKernelGGL((ema_update_kernel<false, kEmaTileCached>),
                       dim3(ema_grid(n4, kEmaTileCached)), dim3(256), 0, st, p, e, n4, t_dev,
                       every, w_min, (int)warmup, scal);
}

void ema_swap(float* p, float* e, void* shadow, long n, hipStream_t st) {
  if (n <= 0) return;
  const long n4 = n / 4;
  if (nt_state())
    hipLaunchKernelGGL((ema_swap_kernel<true, kEmaTileNT>), dim3(ema_grid(n4, kEmaTileNT)),
                       dim3(256), 0, st, p, e, (__bf16*)shadow, n4);
  else
    hipLaunchKernelGGL((ema_swap_kernel<false, kEmaTileCached>),
                       dim3(ema_grid(n4, kEmaTileCached)), dim3(256), 0, st, p, e,
                       (__bf16*)shadow, n4);
}

void ema_buffers_update(const long* table, int nrows, float* eb, long nbuf, const int* t_dev,
                        int every, float w_min, bool warmup, hipStream_t st) {
  if (nrows <= 0) return;
  hipLaunchKernelGGL(ema_buffers_update_kernel, dim3(nrows), dim3(256), 0, st, table, eb, nbuf,
                     t_dev, every, w_min, (int)warmup);
}

void ema_buffers_swap(const long* table, int nrows, float* eb, long nbuf, hipStream_t st) {
  if (nrows <= 0) return;
  hipLaunchKernelGGL(ema_buffers_swap_kernel, dim3(nrows), dim3(256), 0, st, table, eb, nbuf);
}

}  // namespace mipipe
