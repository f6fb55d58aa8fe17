// The optimizers over the flat fp32 parameter buffer, one launch sequence for the whole model,
// each also emitting the bf16 weight shadow: SGD-momentum and AdamW (one grid-stride launch), and
// the layer-wise adaptive LARS and LAMB with global-norm gradient clipping and a learning rate
// that lives on the device.  All of them reach memory through flat_access.hpp, which states the
// access rules (streaming state, cached shadow, loads before uses, no load behind a branch).
//
// LARS / LAMB: the flat buffer is cut into chunks of at most kOptimChunk elements, none crossing
// a segment (parameter) boundary: chunk c = {segment, offset / 64, length, 0}, offset and length
// multiples of 64.  Segment s = {weight decay (float bits), adapt flag, first chunk, chunk
// count}.  A step:
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
#include "flat_access.hpp"

namespace mipipe {

namespace {

// SGD ([torch] optim/sgd.py:354-380): g += wd*p; m = momentum*m + (1-damp)*g (m = g first);
// p -= lr * (nesterov ? g + momentum*m : m).  n % 4 == 0.  Cached accesses, a plain grid-stride
// loop; the momentum load stays behind mom != 0 because m aliases the gradient buffer when the
// momentum is 0.
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ m, __bf16* __restrict__ sh,
                                                  long n4, float lr, float mom, float damp, float wd,
                                                  bool nesterov, bool first, float gs) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 pv = ld4<false>(p, i);
    float4 gv = ld4<false>(g, i);
    float pa[4] = {pv.x, pv.y, pv.z, pv.w};
    float ga[4] = {gv.x * gs, gv.y * gs, gv.z * gs, gv.w * gs};
    if (mom != 0.f) {
      float ma[4];
      unpack(ld4<false>(m, i), ma);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float d = ga[q] + wd * pa[q];
        ma[q] = first ? d : mom * ma[q] + (1.f - damp) * d;
        float upd = nesterov ? d + mom * ma[q] : ma[q];
        pa[q] -= lr * upd;
      }
      st4<false>(m, i, ma);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) pa[q] -= lr * (ga[q] + wd * pa[q]);
    }
    st4<false>(p, i, pa);
    st_shadow(sh, i, pa);
  }
}

// AdamW, grid-stride with U float4 items per thread per iteration (items i0, i0 + stride, ...):
// every item's four loads are issued before any is used.  The first item is in range by the loop
// condition; the later ones are guarded (the items are a grid stride apart, so there is no
// neighbour to clamp to).
template <bool NT, int U>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    __bf16* __restrict__ sh, long n4, float lr,
                                                    float b1, float b2, float eps, float wd,
                                                    float bc1, float bc2, float gs,
                                                    const int* __restrict__ t_dev) {
  if (t_dev != nullptr) {  // step count on the device: graph-replayable bias correction
    const float t = (float)__hip_atomic_load(t_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bc1 = 1.f - exp2f(t * log2f(b1));
    bc2 = 1.f - exp2f(t * log2f(b2));
  }
  const float rbc2 = rsqrtf(bc2);
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < n4; i0 += stride * U) {
    float4 pv[U], gv[U], mv[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (u == 0 || i < n4) {
        pv[u] = ld4<NT>(p, i);
        gv[u] = ld4<NT>(g, i);
        mv[u] = ld4<NT>(m, i);
        vv[u] = ld4<NT>(v, i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + u * stride;
      if (u > 0 && i >= n4) break;
      float pa[4], ga[4], ma[4], va[4];
      unpack(pv[u], pa);
      unpack(gv[u], ga);
      unpack(mv[u], ma);
      unpack(vv[u], va);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float gq = ga[q] * gs;
        pa[q] *= 1.f - lr * wd;
        ma[q] = b1 * ma[q] + (1.f - b1) * gq;
        va[q] = b2 * va[q] + (1.f - b2) * gq * gq;
        float denom = sqrtf(va[q]) * rbc2 + eps;
        pa[q] -= (lr / bc1) * ma[q] / denom;
      }
      st4<NT>(p, i, pa);
      st4<NT>(m, i, ma);
      st4<NT>(v, i, va);
      st_shadow(sh, i, pa);
    }
  }
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

// x0^2 + x1^2 + x2^2 + x3^2 with the roundings spelled out
__device__ __forceinline__ float sumsq(const float (&x)[4]) {
  return __fmaf_rn(x[3], x[3], __fmaf_rn(x[2], x[2], __fmaf_rn(x[0], x[0], x[1] * x[1])));
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

// part[0][c] = sum w^2 (WITH_W, else 0 and p is not read), part[1][c] = sum (g gs)^2 over chunk
// c.  The chunk walk written out, without a branch: a lane past the chunk's end re-reads the
// chunk's last item and adds zero.  It stays written out because its sums are left to the
// compiler's contraction, which follows the shape of this loop: restated on chunk_walk it no
// longer gave the bits it gives here.
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
  for (int r = 0; r < kChunkRounds && r * 256 < len4; r += U) {
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
// (scal null: no clipping).  Each sum of two products is written as the fma it is computed as
// (the first product fused), so the bits do not hang on the compiler's choice of contraction.
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
  float aw = 0.f, au = 0.f;
  chunk_walk<NT, U, 4>(c, {p, g, m, v}, [&](long i, const float4(&x)[4]) {
    float pa[4], ga[4], ma[4], va[4];
    unpack(x[0], pa);
    unpack(x[1], ga);
    unpack(x[2], ma);
    unpack(x[3], va);
    float ua[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float gq = ga[q] * gsc;
      ma[q] = __fmaf_rn(b1, ma[q], omb1 * gq);
      va[q] = __fmaf_rn(b2, va[q], omb2 * gq * gq);
      ua[q] = lamb_u(pa[q], ma[q], va[q], ls, eps, wd);
    }
    aw += sumsq(pa);
    au += sumsq(ua);
    st4<NT>(m, i, ma);
    st4<NT>(v, i, va);
  });
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
// shadow.  The fmas are spelled out as in lamb_moments_kernel.
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
  chunk_walk<NT, U, 3>(c, {p, g, m}, [&](long i, const float4(&x)[3]) {
    float pa[4], ga[4], ma[4];
    unpack(x[0], pa);
    unpack(x[1], ga);
    unpack(x[2], ma);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float d = r * __fmaf_rn(ga[q], gsc, wd * pa[q]);
      ma[q] = __fmaf_rn(mu, ma[q], d);
      pa[q] = __fmaf_rn(-lr, ma[q], pa[q]);
    }
    st4<NT>(p, i, pa);
    st4<NT>(m, i, ma);
    st_shadow(sh, i, pa);
  });
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
  chunk_walk<NT, U, 3>(c, {p, m, v}, [&](long i, const float4(&x)[3]) {
    float pa[4], ma[4], va[4];
    unpack(x[0], pa);
    unpack(x[1], ma);
    unpack(x[2], va);
#pragma unroll
    for (int q = 0; q < 4; ++q) pa[q] -= lrr * lamb_u(pa[q], ma[q], va[q], ls, eps, wd);
    st4<NT>(p, i, pa);
    st_shadow(sh, i, pa);
  });
}

}  // namespace

void sgd_step(float* p, const float* g, float* m, void* shadow, long n, float lr, float momentum,
              float dampening, float wd, bool nesterov, bool first, float grad_scale,
              hipStream_t st) {
  long n4 = n / 4;
  hipLaunchKernelGGL(sgd_kernel, dim3(grid1d(n4, 4)), dim3(256), 0, st, p, g, m, (__bf16*)shadow,
                     n4, lr, momentum, dampening, wd, nesterov, first, grad_scale);
}

void adamw_step(float* p, const float* g, float* m, float* v, void* shadow, long n, float lr,
                float b1, float b2, float eps, float wd, float bc1, float bc2, float grad_scale,
                hipStream_t st, const int* t_dev) {
  long n4 = n / 4;
  // 32768 blocks: 5.10 TB/s at BERT-base size vs 4.63 with the default 8192 cap (more waves in
  // flight per SIMD; tools/r3/adamw_lab.hip, profiles/r3_bert_gemm_splitk_adamw.txt)
  static const int cap = [] {
    const char* e = getenv("MIPIPE_ADAMW_BLOCKS");
    return e == nullptr ? 32768 : atoi(e);
  }();
  // MIPIPE_ADAMW_UNROLL: float4 items in flight per thread (1, 2 or 4); 2 measured +0.7 % on
  // BERT-base over 1 (profiles/r6_adamw_unroll.txt)
  static const int unroll = [] {
    const char* e = getenv("MIPIPE_ADAMW_UNROLL");
    const int u = e != nullptr ? atoi(e) : 2;
    return u == 4 ? 4 : u == 1 ? 1 : 2;
  }();
  dispatch_int<1, 2, 4>(unroll, [&](auto u_c) {
    dispatch_nt([&](auto nt_c) {
      constexpr bool NT = decltype(nt_c)::value;
      constexpr int U = decltype(u_c)::value;
      hipLaunchKernelGGL((adamw_kernel<NT, U>), dim3(grid1d(n4, U, cap)), dim3(256), 0, st, p, g,
                         m, v, (__bf16*)shadow, n4, lr, b1, b2, eps, wd, bc1, bc2, grad_scale,
                         t_dev);
    });
  });
}

void optim_seg_sumsq(const float* p, const float* g, const int* chunks, int nchunks, int nseg,
                     long n, float grad_scale, bool with_w, float* part, hipStream_t st) {
  if (nchunks <= 0) return;
  dispatch_nt([&](auto nt_c) {
    dispatch_bool(with_w, [&](auto w_c) {
      constexpr bool NT = decltype(nt_c)::value;
      constexpr bool W = decltype(w_c)::value;
      hipLaunchKernelGGL((seg_sumsq_kernel<NT, W, 4>), dim3(nchunks), dim3(256), 0, st, p, g,
                         (const int4*)chunks, nchunks, nseg, n, grad_scale, part);
    });
  });
}

void optim_lamb_moments(const float* p, const float* g, float* m, float* v, const int* chunks,
                        const int* segs, int nchunks, int nseg, long n, float grad_scale,
                        float b1, float omb1, float b2, float omb2, float lnb1, float lnb2,
                        float eps, const float* scal, const int* t_dev, float* part,
                        hipStream_t st) {
  if (nchunks <= 0) return;
  dispatch_nt([&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    hipLaunchKernelGGL((lamb_moments_kernel<NT, 2>), dim3(nchunks), dim3(256), 0, st, p, g, m, v,
                       (const int4*)chunks, (const int4*)segs, nchunks, nseg, n, grad_scale, b1,
                       omb1, b2, omb2, lnb1, lnb2, eps, scal, t_dev, part);
  });
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
  dispatch_nt([&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    hipLaunchKernelGGL((lars_apply_kernel<NT, 2>), dim3(nchunks), dim3(256), 0, st, p, g, m,
                       (__bf16*)shadow, (const int4*)chunks, (const int4*)segs, nseg, n,
                       grad_scale, momentum, ratio, scal);
  });
}

void optim_lamb_apply(float* p, const float* m, const float* v, void* shadow, const int* chunks,
                      const int* segs, int nchunks, int nseg, long n, float lnb1, float lnb2,
                      float eps, const float* ratio, const float* scal, const int* t_dev,
                      hipStream_t st) {
  if (nchunks <= 0) return;
  dispatch_nt([&](auto nt_c) {
    constexpr bool NT = decltype(nt_c)::value;
    hipLaunchKernelGGL((lamb_apply_kernel<NT, 2>), dim3(nchunks), dim3(256), 0, st, p, m, v,
                       (__bf16*)shadow, (const int4*)chunks, (const int4*)segs, nseg, n, lnb1,
                       lnb2, eps, ratio, scal, t_dev);
  });
}

}  // namespace mipipe
