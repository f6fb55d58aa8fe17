// Layer-wise adaptive optimizers (LARS, LAMB) over the flat parameter buffer, with global-norm
// gradient clipping and a learning rate that lives on the device.
//
// The flat buffer is cut into chunks of at most kOptimChunk elements, none crossing a segment
// (parameter) boundary: chunk c = {segment, offset / 64, length, 0}, offset and length multiples
// of 64.  Segment s = {weight decay (float bits), adapt flag, first chunk, chunk count}.  A step:
//
//   seg_sumsq / lamb_moments   one block per chunk: the chunk's two partial sums of squares into
//                              part[2][nchunks] (fixed lane tree, wave partials in index order)
//   seg_finish                 one block: per-segment totals, the global gradient norm, the clip
//                              coefficient, the per-segment trust ratios and the step's LR
//   lars_apply / lamb_apply    one block per chunk: the update, reading ratio / clip / LR from
//                              device memory
//
// No float atomics, no host synchronisation, no allocation: per-step scalars (step count, LR,
// clip, ratios) are device memory, so a step captured into a hipGraph replays correctly.
// Padding (alignment tails, reserved pad rows) is zero in p, g, m, v and its update is exactly
// zero under both rules, so it stays zero.
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

constexpr int kItems = kOptimChunk / 4 / 256;  // float4 items per thread of a full chunk
static_assert(kOptimChunk % 1024 == 0, "a chunk is a whole number of 256-thread float4 rounds");

// streaming (non-temporal) access to the fp32 state, touched once per pass (g_nt_store & 1024)
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

// A chunk entry the kernels may act on: inside the buffer, 64-aligned, of a known segment.  The
// host builds the table from FlatParamSpace.ranges(); a block given anything else does nothing.
__device__ __forceinline__ bool chunk_ok(const int4& c, long n, int nseg) {
  return c.x >= 0 && c.x < nseg && c.y >= 0 && c.z > 0 && c.z <= kOptimChunk && (c.z & 63) == 0 &&
         (long)c.y * 64 + c.z <= n;
}

// Block sums of two per-thread values (256 threads): xor butterfly inside each wave (every lane
// ends with the same bits), then the four wave sums added in index order by thread 0.
__device__ __forceinline__ void block_sum2_store(float a, float b, float* out_a, float* out_b) {
  __shared__ float red[2][4];
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *out_a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    *out_b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

__device__ __forceinline__ float sumsq4(const float4& v, float s) {
  const float x = v.x * s, y = v.y * s, z = v.z * s, w = v.w * s;
  return ((x * x + y * y) + z * z) + w * w;
}

// LAMB's per-step scalars from the device step count t: 1 / (1 - beta^t) with
// 1 - beta^t = -expm1(t ln beta) (ln beta comes from the host in double: 1 - beta^t keeps its
// relative precision for beta close to 1, which 1 - exp2(t log2 beta) in fp32 does not).
struct LambStep {
  float rbc1, rbc2;
};
__device__ __forceinline__ LambStep lamb_step_scalars(const int* __restrict__ t_dev, float lnb1,
                                                      float lnb2) {
  const float t = (float)__hip_atomic_load(t_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  LambStep s;
  s.rbc1 = 1.f / -expm1f(t * lnb1);
  s.rbc2 = 1.f / -expm1f(t * lnb2);
  return s;
}

// u = (m / bc1) / (sqrt(v / bc2) + eps) + wd w.  The ONE definition both LAMB passes use, with
// every rounding spelled out (no contraction left to the compiler): the u whose norm gave the
// trust ratio is bit for bit the u that is applied.  w = m = v = 0 gives exactly 0.
__device__ __forceinline__ float lamb_u(float w, float m, float v, const LambStep& s, float eps,
                                        float wd) {
  const float den = __fadd_rn(__fsqrt_rn(__fmul_rn(v, s.rbc2)), eps);
  return __fmaf_rn(wd, w, __fdiv_rn(__fmul_rn(m, s.rbc1), den));
}

// part[0][c] = sum w^2 (WITH_W, else 0), part[1][c] = sum (g gs)^2 over chunk c.  U items of each
// array are loaded before any is used.  No load sits behind a branch (the compiler would close it
// with a full vmcnt(0) drain): a lane past the chunk's end re-reads the chunk's last item and adds
// zero — the same in the kernels below, whose stores alone are conditional.
template <bool NT, bool WITH_W, int U>
__global__ __launch_bounds__(256) void seg_sumsq_kernel(const float* __restrict__ p,
                                                        const float* __restrict__ g,
                                                        const int4* __restrict__ chunks,
                                                        int nchunks, int nseg, long n, float gs,
                                                        float* __restrict__ part) {
  const int4 c = chunks[blockIdx.x];
  if (!chunk_ok(c, n, nseg)) return;
  const long base = (long)c.y * 16;
  const int len4 = c.z >> 2;
  float aw = 0.f, ag = 0.f;
  for (int r = 0; r < kItems && r * 256 < len4; r += U) {
    float4 pv[U], gv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = base + min((r + u) * 256 + (int)threadIdx.x, len4 - 1);
      if constexpr (WITH_W) pv[u] = ld4<NT>(p, j);
      gv[u] = ld4<NT>(g, j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool live = (r + u) * 256 + (int)threadIdx.x < len4;
      if constexpr (WITH_W) aw += sumsq4(pv[u], live ? 1.f : 0.f);
      ag += sumsq4(gv[u], live ? gs : 0.f);
    }
  }
  block_sum2_store(aw, ag, part + blockIdx.x, part + nchunks + blockIdx.x);
}

// LAMB moments: m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) g'^2 in place (g' = g gs clip), and
// part[0][c] = sum w^2, part[1][c] = sum u^2 over chunk c.  scal[1] is the clip coefficient
// (scal null: no clipping).
template <bool NT, int U>
__global__ __launch_bounds__(256) void lamb_moments_kernel(
    const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    float* __restrict__ v, const int4* __restrict__ chunks, const int4* __restrict__ segs,
    int nchunks, int nseg, long n, float gs, float b1, float omb1, float b2, float omb2,
    float lnb1, float lnb2, float eps, const float* __restrict__ scal,
    const int* __restrict__ t_dev, float* __restrict__ part) {
  const int4 c = chunks[blockIdx.x];
  if (!chunk_ok(c, n, nseg)) return;
  const float wd = __int_as_float(segs[c.x].x);
  const float gsc = scal != nullptr ? gs * scal[1] : gs;  // no scal: no clipping
  const LambStep ls = lamb_step_scalars(t_dev, lnb1, lnb2);
  const long base = (long)c.y * 16;
  const int len4 = c.z >> 2;
  float aw = 0.f, au = 0.f;
  for (int r = 0; r < kItems && r * 256 < len4; r += U) {
    float4 pv[U], gv[U], mv[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = base + min((r + u) * 256 + (int)threadIdx.x, len4 - 1);
      pv[u] = ld4<NT>(p, j);
      gv[u] = ld4<NT>(g, j);
      mv[u] = ld4<NT>(m, j);
      vv[u] = ld4<NT>(v, j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = (r + u) * 256 + threadIdx.x;
      if (i >= len4) break;
      const float pa[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
      const float ga[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
      float ma[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
      float va[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
      float sw = 0.f, su = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gq = ga[q] * gsc;
        ma[q] = b1 * ma[q] + omb1 * gq;
        va[q] = b2 * va[q] + omb2 * gq * gq;
        const float uq = lamb_u(pa[q], ma[q], va[q], ls, eps, wd);
        sw += pa[q] * pa[q];
        su += uq * uq;
      }
      aw += sw;
      au += su;
      st4<NT>(m, base + i, ma);
      st4<NT>(v, base + i, va);
    }
  }
  block_sum2_store(aw, au, part + blockIdx.x, part + nchunks + blockIdx.x);
}

// The step's learning rate; step k counts from 0.  Warm-up base (k+1)/W for k < W, then by kind:
// 0 constant, 1 linear, 2 poly (power 2), 3 cosine, from base to end over x = (k-W)/(T-W).
__device__ __forceinline__ float sched_lr(const OptimSched& sc, int k) {
  if (k < sc.warmup) return sc.base * ((float)(k + 1) / (float)sc.warmup);
  if (sc.kind == 0) return sc.base;
  const float x = sc.total > sc.warmup
                      ? fminf(1.f, (float)(k - sc.warmup) / (float)(sc.total - sc.warmup))
                      : 1.f;
  const float f = sc.kind == 1 ? 1.f - x
                  : sc.kind == 2 ? (1.f - x) * (1.f - x)
                                 : 0.5f * (1.f + cospif(x));
  return sc.end + (sc.base - sc.end) * f;
}

// One block of 16 waves.  Wave w owns segments w, w+16, ...: lane l adds the segment's chunk
// partials l, l+64, ... in order, then the fixed lane tree (the assignment and the order never
// depend on timing, as in det_sum_rows_kernel).  Wave 0 then adds the segments' gradient totals
// the same way for the global norm.  scal = {lr, clip, gradient norm}.
//   mode 0 (LARS):       part = {w^2, g^2}: norm, clip, ratio = tc |w| / (clip |g| + wd |w| + eps)
//   mode 1 (clip only):  part = {-, g^2}:   norm, clip
//   mode 2 (LAMB):       part = {w^2, u^2}: ratio = |w| / |u|; clip and norm are left alone
//   mode 3 (LR only):    no partials: ratio = 1, clip = 1
// A ratio is 1 where the segment is not adapted or one of the two norms is 0.
__global__ __launch_bounds__(1024) void seg_finish_kernel(
    const float* __restrict__ part, int nchunks, const int4* __restrict__ segs, int nseg,
    float* __restrict__ segtot, float* __restrict__ ratio, float* __restrict__ scal,
    const int* __restrict__ t_dev, int mode, float tc, float eps, float max_norm,
    OptimSched sc) {
  __shared__ float s_clip;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (mode != 3) {
    for (int s = wave; s < nseg; s += 16) {
      const int4 sg = segs[s];
      float a0 = 0.f, a1 = 0.f;
      if (sg.z >= 0 && sg.w >= 0 && (long)sg.z + sg.w <= nchunks) {
        const float* q = part + sg.z;
#pragma unroll 4
        for (int c = lane; c < sg.w; c += 64) {
          a0 += q[c];
          a1 += q[nchunks + c];
        }
      }
      a0 = wave_sum(a0);
      a1 = wave_sum(a1);
      if (lane == 0) {
        segtot[s] = a0;
        segtot[nseg + s] = a1;
      }
    }
  }
  __syncthreads();  // the segment totals (global memory) are visible to the whole block
  if (wave == 0) {
    float clip = 1.f;
    if (mode == 0 || mode == 1) {
      float a = 0.f;
      for (int s = lane; s < nseg; s += 64) a += segtot[nseg + s];
      const float gn = sqrtf(wave_sum(a));
      if (max_norm > 0.f) clip = fminf(1.f, max_norm / (gn + 1e-6f));
      if (lane == 0) {
        scal[1] = clip;
        scal[2] = gn;
      }
    } else if (mode == 3 && lane == 0) {
      scal[1] = 1.f;
      scal[2] = 0.f;
    }
    if (lane == 0) {
      s_clip = clip;
      const int t = __hip_atomic_load(t_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      scal[0] = sched_lr(sc, t - 1);  // the counter was advanced before the step: step k = t - 1
    }
  }
  __syncthreads();
  if (mode == 1) return;
  const float clip = s_clip;
  for (int s = threadIdx.x; s < nseg; s += 1024) {
    float r = 1.f;
    const int4 sg = segs[s];
    if (mode != 3 && sg.y != 0) {
      const float wn = sqrtf(segtot[s]), on = sqrtf(segtot[nseg + s]);
      if (wn > 0.f && on > 0.f)
        r = mode == 0 ? tc * wn / (clip * on + __int_as_float(sg.x) * wn + eps) : wn / on;
    }
    ratio[s] = r;
  }
}

// LARS: d = r (g' + wd w), m = mu m + d, w -= lr m; g' = g gs clip.  Writes p, m and the bf16
// shadow (cached: the next forward reads it).
template <bool NT, int U>
__global__ __launch_bounds__(256) void lars_apply_kernel(
    float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
    __bf16* __restrict__ sh, const int4* __restrict__ chunks, const int4* __restrict__ segs,
    int nseg, long n, float gs, float mu, const float* __restrict__ ratio,
    const float* __restrict__ scal) {
  const int4 c = chunks[blockIdx.x];
  if (!chunk_ok(c, n, nseg)) return;
  const float wd = __int_as_float(segs[c.x].x);
  const float r = ratio[c.x];
  const float lr = scal[0];
  const float gsc = gs * scal[1];
  const long base = (long)c.y * 16;
  const int len4 = c.z >> 2;
  for (int r0 = 0; r0 < kItems && r0 * 256 < len4; r0 += U) {
    float4 pv[U], gv[U], mv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = base + min((r0 + u) * 256 + (int)threadIdx.x, len4 - 1);
      pv[u] = ld4<NT>(p, j);
      gv[u] = ld4<NT>(g, j);
      mv[u] = ld4<NT>(m, j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = (r0 + u) * 256 + threadIdx.x;
      if (i >= len4) break;
      float pa[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
      const float ga[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
      float ma[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float d = r * (ga[q] * gsc + wd * pa[q]);
        ma[q] = mu * ma[q] + d;
        pa[q] -= lr * ma[q];
      }
      st4<NT>(p, base + i, pa);
      st4<NT>(m, base + i, ma);
      if (sh != nullptr)
        reinterpret_cast<uint2*>(sh)[base + i] =
            make_uint2(pack2(pa[0], pa[1]), pack2(pa[2], pa[3]));
    }
  }
}

// LAMB: w -= lr r u with u recomputed from (w, m, v) by lamb_u — the moments pass stored m and
// v, so the gradient buffer is neither read nor overwritten here.
template <bool NT, int U>
__global__ __launch_bounds__(256) void lamb_apply_kernel(
    float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
    __bf16* __restrict__ sh, const int4* __restrict__ chunks, const int4* __restrict__ segs,
    int nseg, long n, float lnb1, float lnb2, float eps, const float* __restrict__ ratio,
    const float* __restrict__ scal, const int* __restrict__ t_dev) {
  const int4 c = chunks[blockIdx.x];
  if (!chunk_ok(c, n, nseg)) return;
  const float wd = __int_as_float(segs[c.x].x);
  const float lrr = scal[0] * ratio[c.x];
  const LambStep ls = lamb_step_scalars(t_dev, lnb1, lnb2);
  const long base = (long)c.y * 16;
  const int len4 = c.z >> 2;
  for (int r0 = 0; r0 < kItems && r0 * 256 < len4; r0 += U) {
    float4 pv[U], mv[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long j = base + min((r0 + u) * 256 + (int)threadIdx.x, len4 - 1);
      pv[u] = ld4<NT>(p, j);
      mv[u] = ld4<NT>(m, j);
      vv[u] = ld4<NT>(v, j);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = (r0 + u) * 256 + threadIdx.x;
      if (i >= len4) break;
      float pa[4] = {pv[u].x, pv[u].y, pv[u].z, pv[u].w};
      const float ma[4] = {mv[u].x, mv[u].y, mv[u].z, mv[u].w};
      const float va[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
      for (int q = 0; q < 4; ++q) pa[q] -= lrr * lamb_u(pa[q], ma[q], va[q], ls, eps, wd);
      st4<NT>(p, base + i, pa);
      if (sh != nullptr)
        reinterpret_cast<uint2*>(sh)[base + i] =
            make_uint2(pack2(pa[0], pa[1]), pack2(pa[2], pa[3]));
    }
  }
}

inline bool nt_state() { return (g_nt_store & 1024) != 0; }

}  // namespace

void optim_seg_sumsq(const float* p, const float* g, const int* chunks, int nchunks, int nseg,
                     long n, float grad_scale, bool with_w, float* part, hipStream_t st) {
  if (nchunks <= 0) return;
  auto go = [&](auto nt_c, auto w_c) {
    constexpr bool NT = decltype(nt_c)::value;
    constexpr bool W = decltype(w_c)::value;
    hipLaunchKernelGGL((seg_sumsq_kernel<NT, W, 4>), dim3(nchunks), dim3(256), 0, st, p, g,
                       (const int4*)chunks, nchunks, nseg, n, grad_scale, part);
  };
  if (nt_state()) {
    if (with_w) go(std::true_type(), std::true_type());
    else go(std::true_type(), std::false_type());
  } else {
    if (with_w) go(std::false_type(), std::true_type());
    else go(std::false_type(), std::false_type());
  }
}

void optim_lamb_moments(const float* p, const float* g, float* m, float* v, const int* chunks,
                        const int* segs, int nchunks, int nseg, long n, float grad_scale,
                        float b1, float omb1, float b2, float omb2, float lnb1, float lnb2,
                        float eps, const float* scal, const int* t_dev, float* part,
                        hipStream_t st) {
  if (nchunks <= 0) return;
  auto go = [&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    hipLaunchKernelGGL((lamb_moments_kernel<NT, 2>), dim3(nchunks), dim3(256), 0, st, p, g, m, v,
                       (const int4*)chunks, (const int4*)segs, nchunks, nseg, n, grad_scale, b1,
                       omb1, b2, omb2, lnb1, lnb2, eps, scal, t_dev, part);
  };
  if (nt_state()) go(std::true_type());
  else go(std::false_type());
}

void optim_seg_finish(const float* part, int nchunks, const int* segs, int nseg, float* segtot,
                      float* ratio, float* scal, const int* t_dev, int mode, float tc, float eps,
                      float max_norm, const OptimSched& sched, hipStream_t st) {
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(1024), 0, st, part, nchunks,
                     (const int4*)segs, nseg, segtot, ratio, scal, t_dev, mode, tc, eps, max_norm,
                     sched);
}

void optim_lars_apply(float* p, const float* g, float* m, void* shadow, const int* chunks,
                      const int* segs, int nchunks, int nseg, long n, float grad_scale,
                      float momentum, const float* ratio, const float* scal, hipStream_t st) {
  if (nchunks <= 0) return;
  auto go = [&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    hipLaunchKernelGGL((lars_apply_kernel<NT, 2>), dim3(nchunks), dim3(256), 0, st, p, g, m,
                       (__bf16*)shadow, (const int4*)chunks, (const int4*)segs, nseg, n,
                       grad_scale, momentum, ratio, scal);
  };
  if (nt_state()) go(std::true_type());
  else go(std::false_type());
}

void optim_lamb_apply(float* p, const float* m, const float* v, void* shadow, const int* chunks,
                      const int* segs, int nchunks, int nseg, long n, float lnb1, float lnb2,
                      float eps, const float* ratio, const float* scal, const int* t_dev,
                      hipStream_t st) {
  if (nchunks <= 0) return;
  auto go = [&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    hipLaunchKernelGGL((lamb_apply_kernel<NT, 2>), dim3(nchunks), dim3(256), 0, st, p, m, v,
                       (__bf16*)shadow, (const int4*)chunks, (const int4*)segs, nseg, n, lnb1,
                       lnb2, eps, ratio, scal, t_dev);
  };
  if (nt_state()) go(std::true_type());
  else go(std::false_type());
}

}  // namespace mipipe
