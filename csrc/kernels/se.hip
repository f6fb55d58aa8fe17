// Squeeze-excitation and Hardswish kernels (MobileNetV3): BatchNorm apply + ReLU / Hardswish with
// the SE block's global average pool riding in the same pass, its backward as one reduce + one
// apply pass that recompute the pre-activation from y (Hardswish's derivative cannot be read
// from its output) and take the pool's gradient as an addend, and the Hardsigmoid gate multiply
// both ways.  NHWC, T = bf16 | fp32, C % 8 == 0, 16-byte accesses; geometry: launchers.hpp
// (se_slices).  Every elementwise result is a fixed sequence of rounded fp32 operations
// (contraction off: ops/_ref.py reproduces them bit for bit), every sum a fixed-order sum of
// per-block partial rows: the same bits on every launch, in every mode.
#include "common.hpp"
#include "launchers.hpp"

#pragma clang fp contract(off)

namespace mipipe {
namespace {

constexpr int kRelu = kSeActRelu, kHswish = kSeActHardswish;
constexpr int U = kSeRowU;
constexpr int kRedFloats = kSeThreads * 8;  // one [rpb][tpr * 8] array of block partials

struct SeGeom {
  int N, HW, C, C8;
  int tpr, rpb, L, S;
  uint32_t units;  // N * S (sample, slice) pairs
  FastDiv ftpr, fS;
  float inv_hw;
};

inline SeGeom se_geom(int N, int HW, int C) {
  const SeSlices s = se_slices(N, HW, C);
  SeGeom g;
  g.N = N; g.HW = HW; g.C = C; g.C8 = C / 8;
  g.tpr = s.tpr; g.rpb = s.rpb; g.L = s.rows; g.S = s.slices;
  g.units = (uint32_t)N * (uint32_t)s.slices;
  g.ftpr = FastDiv((uint32_t)s.tpr);
  g.fS = FastDiv((uint32_t)s.slices);
  g.inv_hw = (float)(1.0 / (double)HW);
  return g;
}

// A thread's place in the block: row lane rl (clamped into range for addresses), first channel c
// (clamped likewise), live = it owns a real (row lane, channel group), red = its row lane exists
// (it writes its partials, zeros past the last channel group, to the block's LDS rows).
struct SeLane {
  int rl, gi, c;
  bool live, red;
};
__device__ __forceinline__ SeLane se_lane(const SeGeom& g) {
  SeLane l;
  const uint32_t rl0 = g.ftpr.div(threadIdx.x);
  l.gi = (int)(threadIdx.x - rl0 * (uint32_t)g.tpr);
  const int c8 = (int)blockIdx.y * kSeThreads + l.gi;
  l.red = rl0 < (uint32_t)g.rpb;
  l.rl = l.red ? (int)rl0 : g.rpb - 1;
  l.live = l.red && c8 < g.C8;
  l.c = min(c8, g.C8 - 1) * 8;
  return l;
}

// The rows [r0, r1) of unit u = (sample n, slice s)
struct SeUnit {
  uint32_t n;
  int r0, r1;
};
__device__ __forceinline__ SeUnit se_unit(const SeGeom& g, uint32_t u) {
  SeUnit t;
  t.n = g.fS.div(u);
  t.r0 = (int)(u - t.n * (uint32_t)g.S) * g.L;
  t.r1 = min(t.r0 + g.L, g.HW);
  return t;
}

// Column sums of A per-thread accumulators over the block's row lanes, in lane order:
// fin(channel, sums) runs once per channel of the block.
template <int A, class F>
__device__ __forceinline__ void se_block_sums(const float (*acc)[8], float* red, const SeLane& l,
                                              const SeGeom& g, F&& fin) {
  const int cols = g.tpr * 8;
  if (l.red) {
#pragma unroll
    for (int a = 0; a < A; ++a) {
      float4* p = reinterpret_cast<float4*>(red + a * kRedFloats + (l.rl * g.tpr + l.gi) * 8);
      p[0] = make_float4(acc[a][0], acc[a][1], acc[a][2], acc[a][3]);
      p[1] = make_float4(acc[a][4], acc[a][5], acc[a][6], acc[a][7]);
    }
  }
  __syncthreads();
  for (int col = threadIdx.x; col < cols; col += kSeThreads) {
    float s[A];
#pragma unroll
    for (int a = 0; a < A; ++a) s[a] = 0.f;
    for (int k = 0; k < g.rpb; ++k) {
#pragma unroll
      for (int a = 0; a < A; ++a) s[a] += red[a * kRedFloats + k * cols + col];
    }
    const int ch = (int)blockIdx.y * kSeThreads * 8 + col;
    if (ch < g.C) fin(ch, s);
  }
  __syncthreads();
}

// ---- the rounded operations of the contracts ---------------------------------------------------
__device__ __forceinline__ float se_affine(float y, float sc, float bi) {
  const float t = y * sc;
  return t + bi;
}
template <int ACT>
__device__ __forceinline__ float se_act(float u) {
  if constexpr (ACT == kRelu) {
    return fmaxf(u, 0.f);
  } else {
    const float t = fminf(fmaxf(u + 3.f, 0.f), 6.f);
    return (u * t) / 6.f;
  }
}
// e * act'(u) by torch's rules at the knees: ReLU passes u > 0; Hardswish is 0 for u <= -3, the
// slope (u / 3) + 0.5 inside (-3, 3) and 1 for u >= 3 (what ATen's hardswish_backward returns)
template <int ACT>
__device__ __forceinline__ float se_act_grad(float u, float e) {
  if constexpr (ACT == kRelu) {
    return u > 0.f ? e : 0.f;
  } else {
    const float k = (u / 3.f) + 0.5f;
    return u <= -3.f ? 0.f : (u < 3.f ? e * k : e);
  }
}
__device__ __forceinline__ float se_hsigmoid(float v) {
  return fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f;
}
__device__ __forceinline__ float se_hsigmoid_grad(float v) {
  return (v > -3.f && v < 3.f) ? (1.f / 6.f) : 0.f;
}
template <class T>
__device__ __forceinline__ void store1(T* p, float v) { *p = from_f32<T>(v); }

// ---- BatchNorm apply + activation (+ global average pool) --------------------------------------
template <class T, int ACT, bool POOL>
__global__ __launch_bounds__(kSeThreads) void bn_act_pool_fwd_kernel(
    const T* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ bias,
    T* __restrict__ z, float* __restrict__ pm, float* __restrict__ ws, SeGeom g) {
  __shared__ __attribute__((aligned(16))) float red[POOL ? kRedFloats : 4];
  const SeLane l = se_lane(g);
  float sc[8], bi[8];
  ld_f32x8(scale + l.c, sc);
  ld_f32x8(bias + l.c, bi);
  for (uint32_t u = blockIdx.x; u < g.units; u += gridDim.x) {
    const SeUnit t = se_unit(g, u);
    const long base = (long)t.n * g.HW * g.C + l.c;
    float acc[1][8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[0][q] = 0.f;
    for (int rb = t.r0; rb < t.r1; rb += g.rpb * U) {
      Raw8<T> ry[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = min(rb + l.rl + k * g.rpb, t.r1 - 1);
        ry[k] = ld_raw8(y + base + (long)r * g.C);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = rb + l.rl + k * g.rpb;
        const bool ok = l.live && r < t.r1;
        float a[8];
        unpack_raw(ry[k], a);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          a[q] = se_act<ACT>(se_affine(a[q], sc[q], bi[q]));
          if (POOL) acc[0][q] += ok ? as_stored<T>(a[q]) : 0.f;
        }
        if (ok) store8(z + base + (long)r * g.C, a);
      }
    }
    if (POOL) {
      se_block_sums<1>(acc, red, l, g, [&](int ch, const float* s) {
        if (g.S == 1) pm[(long)t.n * g.C + ch] = s[0] * g.inv_hw;
        else ws[(long)u * g.C + ch] = s[0];
      });
    }
  }
}

// pm[n, c] = (sum_s ws[n, s, c]) * (1 / HW), slices in order
__global__ __launch_bounds__(256) void se_pool_finish_kernel(const float* __restrict__ ws,
                                                             float* __restrict__ pm, int NC,
                                                             int C, int S, float inv_hw) {
  const FastDiv fC((uint32_t)C);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < NC; i += gridDim.x * 256) {
    const int n = (int)fC.div((uint32_t)i), c = i - n * C;
    const float* p = ws + (long)n * S * C + c;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += p[(long)k * C];
    pm[i] = s * inv_hw;
  }
}

// ---- its backward: reduce ---------------------------------------------------------------------
template <class T, int ACT, bool DPM>
__global__ __launch_bounds__(kSeThreads) void bn_act_pool_bwd_reduce_kernel(
    const T* __restrict__ dz, const T* __restrict__ y, const float* __restrict__ scale,
    const float* __restrict__ bias, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ dpm, float* __restrict__ ws_g,
    float* __restrict__ ws_gx, SeGeom g) {
  __shared__ __attribute__((aligned(16))) float red[2 * kRedFloats];
  const SeLane l = se_lane(g);
  float sc[8], bi[8], mn[8], is[8], acc[2][8];
  ld_f32x8(scale + l.c, sc);
  ld_f32x8(bias + l.c, bi);
  ld_f32x8(mean + l.c, mn);
  ld_f32x8(invstd + l.c, is);
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[0][q] = acc[1][q] = 0.f;
  for (uint32_t u = blockIdx.x; u < g.units; u += gridDim.x) {
    const SeUnit t = se_unit(g, u);
    const long base = (long)t.n * g.HW * g.C + l.c;
    float dp[8];
    if (DPM) {
      ld_f32x8(dpm + (long)t.n * g.C + l.c, dp);
#pragma unroll
      for (int q = 0; q < 8; ++q) dp[q] = dp[q] * g.inv_hw;
    }
    for (int rb = t.r0; rb < t.r1; rb += g.rpb * U) {
      Raw8<T> rd[U], ry[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = min(rb + l.rl + k * g.rpb, t.r1 - 1);
        rd[k] = ld_raw8(dz + base + (long)r * g.C);
        ry[k] = ld_raw8(y + base + (long)r * g.C);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const bool ok = l.live && rb + l.rl + k * g.rpb < t.r1;
        float d[8], v[8];
        unpack_raw(rd[k], d);
        unpack_raw(ry[k], v);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float uu = se_affine(v[q], sc[q], bi[q]);
          const float e = DPM ? d[q] + dp[q] : d[q];
          const float gg = se_act_grad<ACT>(uu, e);
          const float xh = (v[q] - mn[q]) * is[q];
          const float gx = gg * xh;
          acc[0][q] += ok ? gg : 0.f;
          acc[1][q] += ok ? gx : 0.f;
        }
      }
    }
  }
  se_block_sums<2>(acc, red, l, g, [&](int ch, const float* s) {
    ws_g[(long)blockIdx.x * g.C + ch] = s[0];
    ws_gx[(long)blockIdx.x * g.C + ch] = s[1];
  });
}

// ---- its backward: apply ----------------------------------------------------------------------
template <class T, int ACT, bool DPM, bool SUMS>
__global__ __launch_bounds__(kSeThreads) void bn_act_pool_bwd_apply_kernel(
    const T* __restrict__ dz, const T* __restrict__ y, const float* __restrict__ scale,
    const float* __restrict__ bias, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ dpm, const float* __restrict__ sum_g,
    const float* __restrict__ sum_gx, T* __restrict__ dy, SeGeom g, float inv_cnt) {
  const SeLane l = se_lane(g);
  float sc[8], bi[8], mn[8], is[8], kk[8], mg[8], mgx[8];
  ld_f32x8(scale + l.c, sc);
  ld_f32x8(bias + l.c, bi);
  ld_f32x8(mean + l.c, mn);
  ld_f32x8(invstd + l.c, is);
  ld_f32x8(gamma + l.c, kk);
#pragma unroll
  for (int q = 0; q < 8; ++q) kk[q] = kk[q] * is[q];
  if (SUMS) {
    ld_f32x8(sum_g + l.c, mg);
    ld_f32x8(sum_gx + l.c, mgx);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      mg[q] = mg[q] * inv_cnt;
      mgx[q] = mgx[q] * inv_cnt;
    }
  }
  for (uint32_t u = blockIdx.x; u < g.units; u += gridDim.x) {
    const SeUnit t = se_unit(g, u);
    const long base = (long)t.n * g.HW * g.C + l.c;
    float dp[8];
    if (DPM) {
      ld_f32x8(dpm + (long)t.n * g.C + l.c, dp);
#pragma unroll
      for (int q = 0; q < 8; ++q) dp[q] = dp[q] * g.inv_hw;
    }
    for (int rb = t.r0; rb < t.r1; rb += g.rpb * U) {
      Raw8<T> rd[U], ry[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = min(rb + l.rl + k * g.rpb, t.r1 - 1);
        rd[k] = ld_raw8(dz + base + (long)r * g.C);
        ry[k] = ld_raw8(y + base + (long)r * g.C);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = rb + l.rl + k * g.rpb;
        float d[8], v[8];
        unpack_raw(rd[k], d);
        unpack_raw(ry[k], v);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float uu = se_affine(v[q], sc[q], bi[q]);
          const float e = DPM ? d[q] + dp[q] : d[q];
          const float gg = se_act_grad<ACT>(uu, e);
          if (SUMS) {
            const float xh = (v[q] - mn[q]) * is[q];
            const float a = gg - mg[q];
            const float b = xh * mgx[q];
            d[q] = kk[q] * (a - b);
          } else {
            d[q] = kk[q] * gg;
          }
        }
        if (l.live && r < t.r1) store8(dy + base + (long)r * g.C, d);
      }
    }
  }
}

// ---- the gate multiply ------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(kSeThreads) void se_scale_fwd_kernel(const T* __restrict__ z,
                                                                  const T* __restrict__ gate,
                                                                  T* __restrict__ out, SeGeom g) {
  const SeLane l = se_lane(g);
  for (uint32_t u = blockIdx.x; u < g.units; u += gridDim.x) {
    const SeUnit t = se_unit(g, u);
    const long base = (long)t.n * g.HW * g.C + l.c;
    float s[8];
    load8(gate + (long)t.n * g.C + l.c, s);
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = se_hsigmoid(s[q]);
    for (int rb = t.r0; rb < t.r1; rb += g.rpb * U) {
      Raw8<T> rz[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = min(rb + l.rl + k * g.rpb, t.r1 - 1);
        rz[k] = ld_raw8(z + base + (long)r * g.C);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = rb + l.rl + k * g.rpb;
        float a[8];
        unpack_raw(rz[k], a);
#pragma unroll
        for (int q = 0; q < 8; ++q) a[q] = a[q] * s[q];
        if (l.live && r < t.r1) store8(out + base + (long)r * g.C, a);
      }
    }
  }
}

template <class T>
__global__ __launch_bounds__(kSeThreads) void se_scale_bwd_kernel(
    const T* __restrict__ dout, const T* __restrict__ z, const T* __restrict__ gate,
    T* __restrict__ dz, T* __restrict__ dgate, float* __restrict__ ws, SeGeom g) {
  __shared__ __attribute__((aligned(16))) float red[kRedFloats];
  const SeLane l = se_lane(g);
  for (uint32_t u = blockIdx.x; u < g.units; u += gridDim.x) {
    const SeUnit t = se_unit(g, u);
    const long base = (long)t.n * g.HW * g.C + l.c;
    float s[8], acc[1][8];
    load8(gate + (long)t.n * g.C + l.c, s);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      s[q] = se_hsigmoid(s[q]);
      acc[0][q] = 0.f;
    }
    for (int rb = t.r0; rb < t.r1; rb += g.rpb * U) {
      Raw8<T> rd[U], rz[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = min(rb + l.rl + k * g.rpb, t.r1 - 1);
        rd[k] = ld_raw8(dout + base + (long)r * g.C);
        rz[k] = ld_raw8(z + base + (long)r * g.C);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int r = rb + l.rl + k * g.rpb;
        const bool ok = l.live && r < t.r1;
        float d[8], a[8];
        unpack_raw(rd[k], d);
        unpack_raw(rz[k], a);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float p = d[q] * a[q];
          acc[0][q] += ok ? p : 0.f;
          d[q] = d[q] * s[q];
        }
        if (ok) store8(dz + base + (long)r * g.C, d);
      }
    }
    se_block_sums<1>(acc, red, l, g, [&](int ch, const float* q) {
      const long i = (long)t.n * g.C + ch;
      if (g.S == 1) store1(dgate + i, q[0] * se_hsigmoid_grad(to_f32(gate[i])));
      else ws[(long)u * g.C + ch] = q[0];
    });
  }
}

// dgate[n, c] = T((sum_s ws[n, s, c]) * hardsigmoid'(gate[n, c])), slices in order
template <class T>
__global__ __launch_bounds__(256) void se_gate_finish_kernel(const float* __restrict__ ws,
                                                             const T* __restrict__ gate,
                                                             T* __restrict__ dgate, int NC, int C,
                                                             int S) {
  const FastDiv fC((uint32_t)C);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < NC; i += gridDim.x * 256) {
    const int n = (int)fC.div((uint32_t)i), c = i - n * C;
    const float* p = ws + (long)n * S * C + c;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += p[(long)k * C];
    store1(dgate + i, s * se_hsigmoid_grad(to_f32(gate[i])));
  }
}

inline dim3 se_grid(const SeGeom& g, int cap) {
  return dim3(std::min<uint32_t>(g.units, (uint32_t)cap), (g.C8 + kSeThreads - 1) / kSeThreads);
}
inline int finish_grid(long n) { return (int)std::min<long>((n + 255) / 256, kSeMaxBlocks); }
inline bool se_act_ok(int act) { return act == kRelu || act == kHswish; }

}  // namespace

void bn_act_pool_fwd(const void* y, const float* scale, const float* bias, void* z, float* pm,
                     float* ws, int N, int HW, int C, int act, bool f32, hipStream_t st) {
  if ((long)N * HW * C <= 0 || !se_act_ok(act)) return;
  const SeGeom g = se_geom(N, HW, C);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    dispatch_int<kRelu, kHswish>(act, [&](auto a) {
      dispatch_bool(pm != nullptr, [&](auto p) {
        hipLaunchKernelGGL((bn_act_pool_fwd_kernel<T, decltype(a)::value, decltype(p)::value>),
                           se_grid(g, kSeMaxBlocks), dim3(kSeThreads), 0, st, (const T*)y, scale,
                           bias, (T*)z, pm, ws, g);
      });
    });
  });
  if (pm != nullptr && g.S > 1)
    hipLaunchKernelGGL(se_pool_finish_kernel, dim3(finish_grid((long)N * C)), dim3(256), 0, st, ws,
                       pm, N * C, C, g.S, g.inv_hw);
}

void bn_act_pool_bwd_reduce(const void* dz, const void* y, const float* scale, const float* bias,
                            const float* mean, const float* invstd, const float* dpm, float* ws,
                            float* out_g, float* out_gx, int N, int HW, int C, int act, bool f32,
                            hipStream_t st) {
  if ((long)N * HW * C <= 0 || !se_act_ok(act)) return;
  const SeGeom g = se_geom(N, HW, C);
  const int P = se_reduce_rows(N, HW, C);
  float* ws_gx = ws + (long)P * C;
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    dispatch_int<kRelu, kHswish>(act, [&](auto a) {
      dispatch_bool(dpm != nullptr, [&](auto d) {
        hipLaunchKernelGGL(
            (bn_act_pool_bwd_reduce_kernel<T, decltype(a)::value, decltype(d)::value>),
            se_grid(g, kSeReduceBlocks), dim3(kSeThreads), 0, st, (const T*)dz, (const T*)y, scale,
            bias, mean, invstd, dpm, ws, ws_gx, g);
      });
    });
  });
  det_sum_rows(ws, ws_gx, P, C, out_g, out_gx, false, st);
}

void bn_act_pool_bwd_apply(const void* dz, const void* y, const float* scale, const float* bias,
                           const float* mean, const float* invstd, const float* gamma,
                           const float* dpm, const float* sum_g, const float* sum_gx, void* dy,
                           int N, int HW, int C, int act, bool f32, hipStream_t st) {
  if ((long)N * HW * C <= 0 || !se_act_ok(act)) return;
  const SeGeom g = se_geom(N, HW, C);
  const float inv_cnt = (float)(1.0 / ((double)N * (double)HW));
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    dispatch_int<kRelu, kHswish>(act, [&](auto a) {
      dispatch_bool(dpm != nullptr, [&](auto d) {
        dispatch_bool(sum_g != nullptr, [&](auto s) {
          hipLaunchKernelGGL((bn_act_pool_bwd_apply_kernel<T, decltype(a)::value,
                                                           decltype(d)::value, decltype(s)::value>),
                             se_grid(g, kSeMaxBlocks), dim3(kSeThreads), 0, st, (const T*)dz,
                             (const T*)y, scale, bias, mean, invstd, gamma, dpm, sum_g, sum_gx,
                             (T*)dy, g, inv_cnt);
        });
      });
    });
  });
}

void se_scale_fwd(const void* z, const void* gate, void* out, int N, int HW, int C, bool f32,
                  hipStream_t st) {
  if ((long)N * HW * C <= 0) return;
  const SeGeom g = se_geom(N, HW, C);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(se_scale_fwd_kernel<T>, se_grid(g, kSeMaxBlocks), dim3(kSeThreads), 0, st,
                       (const T*)z, (const T*)gate, (T*)out, g);
  });
}

void se_scale_bwd(const void* dout, const void* z, const void* gate, void* dz, void* dgate,
                  float* ws, int N, int HW, int C, bool f32, hipStream_t st) {
  if ((long)N * HW * C <= 0) return;
  const SeGeom g = se_geom(N, HW, C);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(se_scale_bwd_kernel<T>, se_grid(g, kSeMaxBlocks), dim3(kSeThreads), 0, st,
                       (const T*)dout, (const T*)z, (const T*)gate, (T*)dz, (T*)dgate, ws, g);
    if (g.S > 1)
      hipLaunchKernelGGL(se_gate_finish_kernel<T>, dim3(finish_grid((long)N * C)), dim3(256), 0,
                         st, ws, (const T*)gate, (T*)dgate, N * C, C, g.S);
  });
}

}  // namespace mipipe
