// Vision Transformer input side: the passes between the NCHW image and the encoder's token
// stream that are neither a GEMM nor a LayerNorm.
//
//   patchify            x [B, C, H, W] (fp32 / bf16) -> tok [B*gh*gw, C*P*P] (bf16 / fp32):
//                       row (b, i, j), column (c, u, v) = x[b, c, i*P + u, j*P + v].  The column
//                       order is that of conv_proj.weight.view(D, C*P*P), so the P x P stride-P
//                       convolution is the GEMM tok @ weight^T on the parameter as it stands.
//                       A permutation and one rounding: no arithmetic.
//   tokens_assemble_fwd h[b, 0] = cls + pos[0], h[b, 1 + n] = e[b, n] + pos[1 + n]: one fp32 add,
//                       one rounding to the activation type.
//   tokens_assemble_bwd de = dh[:, 1:] (compact copy), dpos[s] += sum_b dh[b, s],
//                       dcls += sum_b dh[b, 0].  One thread owns 8 columns of one token position
//                       and walks the batch in ascending b: no atomics, no partial rows, so the
//                       sums have the same bits in every run and every mode.
//
// Streaming passes: one work item is 8 consecutive elements (16 bytes of bf16, two 16-byte
// accesses of fp32).  A block takes whole tiles of kItems items per thread with every load issued
// before the first store; only the last, partial tile checks its items one by one.
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

constexpr int kVitThreads = 256;
constexpr int kVitMaxBlocks = 2048;
constexpr int kItems = 4;  // items per thread and tile: their loads are in flight together

// ------------------------------------------------------------------------------ patchify
struct PatchGeom {
  FastDiv fP8, fP, fC, fgw, fgh;  // P / 8, P, C, W / P, H / P
  int C, H, W, P;
};

// element offset in x of output item o (8 consecutive v of one patch row)
__device__ __forceinline__ long patch_src(const PatchGeom& g, uint32_t o) {
  uint32_t t = g.fP8.div(o);
  const uint32_t v8 = o - t * g.fP8.d;
  uint32_t q = g.fP.div(t);
  const uint32_t u = t - q * g.fP.d;
  t = g.fC.div(q);
  const uint32_t c = q - t * g.fC.d;
  q = g.fgw.div(t);
  const uint32_t j = t - q * g.fgw.d;
  const uint32_t b = g.fgh.div(q);
  const uint32_t i = q - b * g.fgh.d;
  const long row = ((long)b * g.C + c) * g.H + (long)i * g.P + u;
  return row * g.W + (long)j * g.P + v8 * 8;
}

template <class TI, class TO>
__global__ __launch_bounds__(kVitThreads) void patchify_kernel(const TI* __restrict__ x,
                                                               TO* __restrict__ out,
                                                               uint32_t items, PatchGeom g) {
  constexpr uint32_t kTile = kVitThreads * kItems;
  for (uint32_t t0 = blockIdx.x * kTile; t0 < items; t0 += gridDim.x * kTile) {
    const uint32_t o0 = t0 + threadIdx.x;
    if (t0 + kTile <= items) {  // full tile (block-uniform): no per-lane bound on the loads
      Raw8<TI> r[kItems];
#pragma unroll
      for (int k = 0; k < kItems; ++k) r[k] = ld_raw8(x + patch_src(g, o0 + k * kVitThreads));
#pragma unroll
      for (int k = 0; k < kItems; ++k) {
        float f[8];
        unpack_raw(r[k], f);
        store8(out + (long)(o0 + k * kVitThreads) * 8, f);
      }
    } else {
      for (uint32_t o = o0; o < items; o += kVitThreads) {
        float f[8];
        unpack_raw(ld_raw8(x + patch_src(g, o)), f);
        store8(out + (long)o * 8, f);
      }
    }
  }
}

// P == 4 (ConvNeXt's stem): 8 output columns are two 4-pixel patch rows (c, u, 0..3), (c, u + 1,
// 0..3) with u even, i.e. two 4-element source runs one image row apart: 8-byte (bf16) / 16-byte
// (fp32) loads, one 16-byte store per 8 bf16.
__device__ __forceinline__ void ld4(const __bf16* p, float* f) {
  unpack4(*reinterpret_cast<const uint2*>(p), f);
}
__device__ __forceinline__ void ld4(const float* p, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
}

template <class TI, class TO>
__global__ __launch_bounds__(kVitThreads) void patchify4_kernel(const TI* __restrict__ x,
                                                                TO* __restrict__ out,
                                                                uint32_t items, FastDiv fC2,
                                                                FastDiv fgw, FastDiv fgh, int C,
                                                                int H, int W) {
  constexpr uint32_t kTile = kVitThreads * kItems;
  for (uint32_t t0 = blockIdx.x * kTile; t0 < items; t0 += gridDim.x * kTile) {
    float f[kItems][8];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {  // the tail's lanes re-read the last item (valid memory)
      const uint32_t o = min(t0 + threadIdx.x + k * kVitThreads, items - 1);
      const uint32_t r = fC2.div(o);  // output row (b, i, j)
      const uint32_t cu = o - r * fC2.d;
      const uint32_t c = cu >> 1, u = (cu & 1) * 2;
      const uint32_t t = fgw.div(r);
      const uint32_t j = r - t * fgw.d;
      const uint32_t b = fgh.div(t);
      const uint32_t i = t - b * fgh.d;
      const long src = ((((long)b * C + c) * H + i * 4 + u) * W) + (long)j * 4;
      ld4(x + src, f[k]);
      ld4(x + src + W, f[k] + 4);
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const uint32_t o = t0 + threadIdx.x + k * kVitThreads;
      if (o < items) store8(out + (long)o * 8, f[k]);
    }
  }
}

// --------------------------------------------------------------------- tokens_assemble_fwd
template <class T>
__global__ __launch_bounds__(kVitThreads) void tokens_fwd_kernel(
    const T* __restrict__ e, const float* __restrict__ cls, const float* __restrict__ pos,
    T* __restrict__ h, uint32_t items, int N, int D, FastDiv fD8, FastDiv fS) {
  constexpr uint32_t kTile = kVitThreads * kItems;
  // item o: 8 columns at d of output row r = b * (N + 1) + s.  Row s = 0 has no e row: its lanes
  // load the sample's first e row like their neighbours (valid memory, value unused) and take
  // the class token instead, so the e / pos loads of a tile sit behind no per-lane branch.
  auto src = [&](uint32_t o, long& eoff, uint32_t& s, uint32_t& d) {
    const uint32_t r = fD8.div(o);
    d = (o - r * fD8.d) * 8;
    const uint32_t b = fS.div(r);
    s = r - b * fS.d;
    eoff = ((long)b * N + (s == 0 ? 0 : s - 1)) * D + d;
  };
  auto finish = [&](const Raw8<T>& re, const Raw8<float>& rp, uint32_t o, uint32_t s, uint32_t d) {
    float a[8], p[8];
    unpack_raw(re, a);
    unpack_raw(rp, p);
    if (s == 0) ld_f32x8(cls + d, a);
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] += p[q];
    store8(h + (long)o * 8, a);
  };
  for (uint32_t t0 = blockIdx.x * kTile; t0 < items; t0 += gridDim.x * kTile) {
    const uint32_t o0 = t0 + threadIdx.x;
    if (t0 + kTile <= items) {
      Raw8<T> re[kItems];
      Raw8<float> rp[kItems];
      uint32_t s[kItems], d[kItems];
#pragma unroll
      for (int k = 0; k < kItems; ++k) {
        long eoff;
        src(o0 + k * kVitThreads, eoff, s[k], d[k]);
        re[k] = ld_raw8(e + eoff);
        rp[k] = ld_raw8(pos + (long)s[k] * D + d[k]);
      }
#pragma unroll
      for (int k = 0; k < kItems; ++k) finish(re[k], rp[k], o0 + k * kVitThreads, s[k], d[k]);
    } else {
      for (uint32_t o = o0; o < items; o += kVitThreads) {
        long eoff;
        uint32_t s, d;
        src(o, eoff, s, d);
        finish(ld_raw8(e + eoff), ld_raw8(pos + (long)s * D + d), o, s, d);
      }
    }
  }
}

// --------------------------------------------------------------------- tokens_assemble_bwd
constexpr int kTokBwdThreads = 64;  // one wave per block: the few owners spread over all CUs
constexpr int kTokBwdRows = 8;      // batch rows whose loads are in flight per thread

// Thread = 8 columns at d of token position s, all B samples in ascending b.
template <class T>
__global__ __launch_bounds__(kTokBwdThreads) void tokens_bwd_kernel(
    const T* __restrict__ dh, T* __restrict__ de, float* __restrict__ dpos,
    float* __restrict__ dcls, int B, int N, int D, uint32_t owners, FastDiv fD8) {
  const uint32_t o = blockIdx.x * kTokBwdThreads + threadIdx.x;
  if (o >= owners) return;
  const uint32_t s = fD8.div(o);
  const uint32_t d = (o - s * fD8.d) * 8;
  const long sstride = (long)(N + 1) * D;  // one sample of dh
  const long estride = (long)N * D;        // one sample of de
  const T* src = dh + (long)s * D + d;
  T* dst = de + (long)(s == 0 ? 0 : s - 1) * D + d;  // written for s >= 1 only
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.f;
  auto take = [&](const Raw8<T>& r, int b) {
    float f[8];
    unpack_raw(r, f);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] += f[q];
    if (s != 0) store8(dst + (long)b * estride, f);  // bf16 -> fp32 -> bf16 keeps the bits
  };
  int b = 0;
  for (; b + kTokBwdRows <= B; b += kTokBwdRows) {
    Raw8<T> r[kTokBwdRows];
#pragma unroll
    for (int k = 0; k < kTokBwdRows; ++k) r[k] = ld_raw8(src + (long)(b + k) * sstride);
#pragma unroll
    for (int k = 0; k < kTokBwdRows; ++k) take(r[k], b + k);
  }
  for (; b < B; ++b) take(ld_raw8(src + (long)b * sstride), b);
  float cur[8];
  ld_f32x8(dpos + (long)s * D + d, cur);
#pragma unroll
  for (int q = 0; q < 8; ++q) cur[q] += acc[q];
  store8(dpos + (long)s * D + d, cur);
  if (s == 0) {
    ld_f32x8(dcls + d, cur);
#pragma unroll
    for (int q = 0; q < 8; ++q) cur[q] += acc[q];
    store8(dcls + d, cur);
  }
}

inline int vit_grid(uint32_t items) {
  const uint32_t tile = kVitThreads * kItems;
  return (int)std::max<uint32_t>(1, std::min<uint32_t>((items + tile - 1) / tile, kVitMaxBlocks));
}

}  // namespace

void patchify(const void* x, void* out, int B, int C, int H, int W, int P, bool in_f32,
              bool out_f32, hipStream_t st) {
  const long n = (long)B * C * H * W;
  if (n <= 0) return;
  const uint32_t items = (uint32_t)(n / 8);
  if (P == 4) {
    const FastDiv fC2((uint32_t)C * 2), fgw((uint32_t)(W / 4)), fgh((uint32_t)(H / 4));
    dispatch_act(in_f32, [&](auto ti) {
      dispatch_act(out_f32, [&](auto to) {
        using TI = decltype(ti);
        using TO = decltype(to);
        hipLaunchKernelGGL((patchify4_kernel<TI, TO>), dim3(vit_grid(items)), dim3(kVitThreads),
                           0, st, (const TI*)x, (TO*)out, items, fC2, fgw, fgh, C, H, W);
      });
    });
    return;
  }
  PatchGeom g;
  g.fP8 = FastDiv((uint32_t)P / 8);
  g.fP = FastDiv((uint32_t)P);
  g.fC = FastDiv((uint32_t)C);
  g.fgw = FastDiv((uint32_t)(W / P));
  g.fgh = FastDiv((uint32_t)(H / P));
  g.C = C;
  g.H = H;
  g.W = W;
  g.P = P;
  dispatch_act(in_f32, [&](auto ti) {
    dispatch_act(out_f32, [&](auto to) {
      using TI = decltype(ti);
      using TO = decltype(to);
      hipLaunchKernelGGL((patchify_kernel<TI, TO>), dim3(vit_grid(items)), dim3(kVitThreads), 0,
                         st, (const TI*)x, (TO*)out, items, g);
    });
  });
}

void tokens_assemble_fwd(const void* e, const float* cls, const float* pos, void* h, int B, int N,
                         int D, bool f32, hipStream_t st) {
  const long n = (long)B * (N + 1) * D;
  if (n <= 0) return;
  const uint32_t items = (uint32_t)(n / 8);
  const FastDiv fD8((uint32_t)D / 8), fS((uint32_t)(N + 1));
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(tokens_fwd_kernel<T>, dim3(vit_grid(items)), dim3(kVitThreads), 0, st,
                       (const T*)e, cls, pos, (T*)h, items, N, D, fD8, fS);
  });
}

void tokens_assemble_bwd(const void* dh, void* de, float* dpos, float* dcls, int B, int N, int D,
                         bool f32, hipStream_t st) {
  if (B <= 0 || D <= 0) return;
  const uint32_t owners = (uint32_t)((long)(N + 1) * (D / 8));
  const int grid = (int)((owners + kTokBwdThreads - 1) / kTokBwdThreads);
  const FastDiv fD8((uint32_t)D / 8);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(tokens_bwd_kernel<T>, dim3(grid), dim3(kTokBwdThreads), 0, st,
                       (const T*)dh, (T*)de, dpos, dcls, B, N, D, owners, fD8);
  });
}

}  // namespace mipipe
