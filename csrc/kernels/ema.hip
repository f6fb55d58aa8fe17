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
#include "flat_access.hpp"

namespace mipipe {

namespace {

// float4 items per block, measured at the ResNet-50 and BERT-base flat sizes with the buffers not
// in the memory-side cache (profiles/model_ema.txt): streaming accesses are fastest with four
// items of each array in flight per thread and no loop, cached accesses with one (many small
// blocks, as ATen's elementwise kernels have them).  Larger tiles and persistent grids lost 2-7 %.
constexpr int kEmaTileNT = 1024;
constexpr int kEmaTileCached = 256;

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

template <bool NT, int TILE4>
__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p,
                                                         float* __restrict__ e, long n4,
                                                         const int* __restrict__ t_dev, int every,
                                                         float w_min, int warmup,
                                                         float* __restrict__ scal) {
  float w;
  if (!ema_weight(t_dev, every, w_min, warmup, &w)) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) scal[0] = w;
  tile_walk<NT, TILE4, 2>(n4, {p, e}, [&](long i, const float4(&x)[2]) {
    const float4 &pv = x[0], &ev = x[1];
    const float ea[4] = {ema_lerp(ev.x, pv.x, w), ema_lerp(ev.y, pv.y, w),
                         ema_lerp(ev.z, pv.z, w), ema_lerp(ev.w, pv.w, w)};
    st4<NT>(e, i, ea);
  });
}

// p and e exchanged; the bf16 shadow of the new p written with the optimizer kernels' conversion
template <bool NT, int TILE4>
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p,
                                                       float* __restrict__ e,
                                                       __bf16* __restrict__ sh, long n4) {
  tile_walk<NT, TILE4, 2>(n4, {p, e}, [&](long i, const float4(&x)[2]) {
    float pa[4], ea[4];
    unpack(x[0], pa);
    unpack(x[1], ea);
    st4<NT>(p, i, ea);
    st4<NT>(e, i, pa);
    st_shadow(sh, i, ea);
  });
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

inline int ema_grid(long n4, int tile4) { return (int)((n4 + tile4 - 1) / tile4); }

}  // namespace

void ema_update(const float* p, float* e, long n, const int* t_dev, int every, float w_min,
                bool warmup, float* scal, hipStream_t st) {
  if (n <= 0) return;
  const long n4 = n / 4;
  dispatch_nt([&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    constexpr int T = NT ? kEmaTileNT : kEmaTileCached;
    hipLaunchKernelGGL((ema_update_kernel<NT, T>), dim3(ema_grid(n4, T)), dim3(256), 0, st, p, e,
                       n4, t_dev, every, w_min, (int)warmup, scal);
  });
}

void ema_swap(float* p, float* e, void* shadow, long n, hipStream_t st) {
  if (n <= 0) return;
  const long n4 = n / 4;
  dispatch_nt([&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    constexpr int T = NT ? kEmaTileNT : kEmaTileCached;
    hipLaunchKernelGGL((ema_swap_kernel<NT, T>), dim3(ema_grid(n4, T)), dim3(256), 0, st, p, e,
                       (__bf16*)shadow, n4);
  });
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
