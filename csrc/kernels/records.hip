// Record decode: the device side of the record loader (csrc/runtime/loader.cpp RecordLoader::fill).
// Input: whole uint8 records ([label bytes][C planes of H*W uint8], any stride, nothing aligned)
// as the loader's raw mode uploads them, plus the global sample indices.  Output: the cropped /
// flipped / normalised NCHW batch (fp32 or bf16) and the int64 labels — element for element what
// fill() writes: the augmentation is splitmix64 of (seed, epoch, sample index), padding pixels are
// zero before the normalisation, and v * scale + offset is a rounded multiply followed by a
// rounded add (the host build has no FMA), so the fp32 output equals the host loader's bit for bit.
//
// A streaming pass (1 B in, 4 or 2 B out per element): a block works on one sample, thread 0
// derives (dy, dx, flip) once, consecutive lanes write consecutive V-element groups of an output
// row (16 B per lane when W allows it, 8 B for bf16 rows of W % 4 == 0, else one element) and
// the flip reverses the read side.
//
// record_decode_rrc (second half of the file) is the resizing transform, "rrc": the same records
// in, a RandomResizedCrop / centre-crop box resampled bilinearly to Ho x Wo out.
#include "../common/rrc.hpp"
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// v * sc + off in two roundings like the host build (g++ -O2, no FMA).  hipcc contracts a
// multiply and an add into v_fma_f32 by default — also through __fmul_rn / __fadd_rn, which are
// plain operators in HIP — so contraction is switched off for this expression.
__device__ __forceinline__ float scale_offset(float v, float sc, float off) {
#pragma clang fp contract(off)
  const float m = v * sc;
  return m + off;
}

template <int V>
__device__ __forceinline__ void store_row(float* p, const float* f) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
  else p[0] = f[0];
}
template <int V>
__device__ __forceinline__ void store_row(__bf16* p, const float* f) {
  if constexpr (V == 8) *reinterpret_cast<uint4*>(p) = pack8(f);
  else if constexpr (V == 4) *reinterpret_cast<uint2*>(p) = pack4(f);
  else p[0] = (__bf16)f[0];  // round to nearest even
}

constexpr int kThreads = 256;

template <class T, int V>
__global__ __launch_bounds__(kThreads) void record_decode_kernel(
    const uint8_t* __restrict__ rec, const int64_t* __restrict__ idx,
    const float* __restrict__ affine, T* __restrict__ x, int64_t* __restrict__ y, long n, int C,
    int H, int W, int label_bytes, long rec_bytes, uint64_t seed, uint64_t epoch, int pad,
    int flip, int train, int parts) {
  __shared__ int s_aug[3];
  const int Wv = W / V;
  const int items = C * H * Wv;  // V-element groups of one sample
  const long per = (long)C * H * W;
  const long units = n * parts;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long s = u / parts;
    const int part = (int)(u - s * parts);
    const uint8_t* r = rec + s * rec_bytes;
    if (threadIdx.x == 0) {
      int dy = 0, dx = 0, fl = 0;
      if (train) {
        const uint64_t h = splitmix64(seed ^ splitmix64(epoch * 0x100000001b3ull ^ (uint64_t)idx[s]));
        if (pad > 0) {
          dy = (int)(h % (uint64_t)(2 * pad + 1)) - pad;
          dx = (int)((h >> 16) % (uint64_t)(2 * pad + 1)) - pad;
        }
        fl = flip && ((h >> 40) & 1);
      }
      s_aug[0] = dy;
      s_aug[1] = dx;
      s_aug[2] = fl;
      if (part == 0) {
        int64_t label = 0;
        for (int k = 0; k < label_bytes; ++k) label |= (int64_t)r[k] << (8 * k);
        y[s] = label;
      }
    }
    __syncthreads();
    const int dy = s_aug[0], dx = s_aug[1], fl = s_aug[2];
    const uint8_t* img = r + label_bytes;
    T* xs = x + s * per;
    for (int it = part * kThreads + (int)threadIdx.x; it < items; it += parts * kThreads) {
      const int row = it / Wv;  // c * H + y
      const int x0 = (it - row * Wv) * V;
      const int c = row / H;
      const int sy = row - c * H + dy;
      const float sc = affine[c], off = affine[C + c];
      const bool row_ok = sy >= 0 && sy < H;
      const uint8_t* ip = img + ((long)c * H + sy) * W;
      float f[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const int xx = fl ? W - 1 - (x0 + j) : x0 + j;
        const int sx = xx + dx;
        const float v = (row_ok && sx >= 0 && sx < W) ? (float)ip[sx] : 0.f;
        f[j] = scale_offset(v, sc, off);
      }
      store_row<V>(xs + (long)row * W + x0, f);
    }
    __syncthreads();  // s_aug is rewritten by the next unit
  }
}

template <class T, int V>
void launch(const uint8_t* rec, const int64_t* idx, const float* affine, void* x, int64_t* y,
            long n, int C, int H, int W, int label_bytes, uint64_t seed, uint64_t epoch, int pad,
            bool flip, bool train, hipStream_t st) {
  const long items = (long)C * H * (W / V);
  const int parts = (int)std::min<long>(32, (items + kThreads - 1) / kThreads);
  const long units = n * parts;
  const unsigned grid = (unsigned)std::min<long>(units, 1l << 20);
  const long rec_bytes = (long)label_bytes + (long)C * H * W;
  hipLaunchKernelGGL((record_decode_kernel<T, V>), dim3(grid), dim3(kThreads), 0, st, rec, idx,
                     affine, (T*)x, y, n, C, H, W, label_bytes, rec_bytes, seed, epoch, pad,
                     (int)flip, (int)train, parts);
}

// ------------------------------------------------------------------------------------- "rrc"
// RandomResizedCrop + flip + Normalize (train) / 7/8 centre crop (eval) to Ho x Wo: the device
// side of RecordLoader::fill_rrc, geometry from common/rrc.hpp.  A block works on one sample:
// thread 0 derives the box, then the block builds two LDS tables — the Ho row taps and the Wo
// column taps with the flip folded in, each entry (absolute source index of tap 0, Q16 weight of
// tap 1 | (tap 1 is a different pixel) << 16) — so the 64-bit divisions are Ho + Wo per block
// and the inner loop is four byte loads, the exact horizontal blends and three rounded operations
// per element.  A lane owns V consecutive output columns of a row (16-byte stores).
__device__ __forceinline__ float blend_rows(float top, float ly0, float bot, float ly1) {
#pragma clang fp contract(off)
  const float a = top * ly0;
  const float b = bot * ly1;
  return a + b;
}

template <class T, int V>
__global__ __launch_bounds__(kThreads) void record_decode_rrc_kernel(
    const uint8_t* __restrict__ rec, const int64_t* __restrict__ idx,
    const float* __restrict__ affine, T* __restrict__ x, int64_t* __restrict__ y, long n, int C,
    int H, int W, int Ho, int Wo, int label_bytes, long rec_bytes, uint64_t seed, uint64_t epoch,
    int flip, int train, int parts) {
  extern __shared__ uint2 s_tap[];  // [0, Ho): rows, [Ho, Ho + Wo): columns
  __shared__ mipipe_rrc::Box s_box;
  const int Wv = Wo / V;
  const int items = C * Ho * Wv;  // V-element groups of one sample
  const long per = (long)C * Ho * Wo;
  const long units = n * parts;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long s = u / parts;
    const int part = (int)(u - s * parts);
    const uint8_t* r = rec + s * rec_bytes;
    if (threadIdx.x == 0) {
      s_box = mipipe_rrc::rrc_box(seed, epoch, (uint64_t)idx[s], H, W, train != 0, flip != 0);
      if (part == 0) {
        int64_t label = 0;
        for (int k = 0; k < label_bytes; ++k) label |= (int64_t)r[k] << (8 * k);
        y[s] = label;
      }
    }
    __syncthreads();
    const mipipe_rrc::Box bx = s_box;
    for (int t = (int)threadIdx.x; t < Ho + Wo; t += kThreads) {
      mipipe_rrc::Tap tp;
      int base;
      if (t < Ho) {
        tp = mipipe_rrc::rrc_tap(t, bx.h, Ho);
        base = bx.y0;
      } else {
        const int ox = t - Ho;
        tp = mipipe_rrc::rrc_tap(bx.flip ? Wo - 1 - ox : ox, bx.w, Wo);
        base = bx.x0;
      }
      s_tap[t] = make_uint2((unsigned)(base + tp.i0), tp.frac | ((unsigned)(tp.i1 - tp.i0) << 16));
    }
    __syncthreads();
    const uint8_t* img = r + label_bytes;
    T* xs = x + s * per;
    for (int it = part * kThreads + (int)threadIdx.x; it < items; it += parts * kThreads) {
      const int row = it / Wv;  // c * Ho + oy
      const int xg = (it - row * Wv) * V;
      const int c = row / Ho;
      const int oy = row - c * Ho;
      const float sc = affine[c], off = affine[C + c];
      const uint2 ty = s_tap[oy];
      const float ly1 = (float)(ty.y & 0xffffu) * (1.f / 65536.f), ly0 = 1.f - ly1;
      const uint8_t* r0 = img + ((long)c * H + ty.x) * W;
      const uint8_t* r1 = r0 + (long)(ty.y >> 16) * W;
      float f[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const uint2 tx = s_tap[Ho + xg + j];
        const float lx1 = (float)(tx.y & 0xffffu) * (1.f / 65536.f), lx0 = 1.f - lx1;
        const unsigned c0 = tx.x, c1 = tx.x + (tx.y >> 16);
        // 8-bit pixels times Q16 weights that sum to 1: exact in fp32 in any evaluation order
        const float top = (float)r0[c0] * lx0 + (float)r0[c1] * lx1;
        const float bot = (float)r1[c0] * lx0 + (float)r1[c1] * lx1;
        f[j] = scale_offset(blend_rows(top, ly0, bot, ly1), sc, off);
      }
      store_row<V>(xs + (long)row * Wo + xg, f);
    }
    __syncthreads();  // s_box and s_tap are rewritten by the next unit
  }
}

template <class T, int V>
void launch_rrc(const uint8_t* rec, const int64_t* idx, const float* affine, void* x, int64_t* y,
                long n, int C, int H, int W, int Ho, int Wo, int label_bytes, uint64_t seed,
                uint64_t epoch, bool flip, bool train, hipStream_t st) {
  const long items = (long)C * Ho * (Wo / V);
  // every part rebuilds the sample's tables: give it at least 8 items per thread
  const int parts = (int)std::max<long>(1, std::min<long>(32, items / (8 * kThreads)));
  const long units = n * parts;
  const unsigned grid = (unsigned)std::min<long>(units, 1l << 20);
  const long rec_bytes = (long)label_bytes + (long)C * H * W;
  const size_t lds = (size_t)(Ho + Wo) * sizeof(uint2);
  hipLaunchKernelGGL((record_decode_rrc_kernel<T, V>), dim3(grid), dim3(kThreads), lds, st, rec,
                     idx, affine, (T*)x, y, n, C, H, W, Ho, Wo, label_bytes, rec_bytes, seed,
                     epoch, (int)flip, (int)train, parts);
}

// f(T{}, V) for the output dtype and the widest row vector that divides the output width w:
// 16 bytes (8 bf16 / 4 fp32), else 4 elements, else 1
template <class F>
void dispatch_row_vec(bool bf16_out, int w, F&& f) {
  dispatch_act(!bf16_out, [&](auto t) {
    constexpr int VMAX = 16 / (int)sizeof(t);
    dispatch_int<VMAX, 4, 1>(w % VMAX == 0 ? VMAX : w % 4 == 0 ? 4 : 1,
                             [&](auto v_c) { f(t, v_c); });
  });
}

}  // namespace

void record_decode_rrc(const uint8_t* rec, const int64_t* idx, const float* affine, void* x,
                       bool bf16_out, int64_t* y, long n, int C, int H, int W, int Ho, int Wo,
                       int label_bytes, uint64_t seed, uint64_t epoch, bool flip, bool train,
                       hipStream_t st) {
  if (n <= 0) return;
  dispatch_row_vec(bf16_out, Wo, [&](auto t, auto v_c) {
    launch_rrc<decltype(t), decltype(v_c)::value>(rec, idx, affine, x, y, n, C, H, W, Ho, Wo,
                                                  label_bytes, seed, epoch, flip, train, st);
  });
}

void record_decode(const uint8_t* rec, const int64_t* idx, const float* affine, void* x,
                   bool bf16_out, int64_t* y, long n, int C, int H, int W, int label_bytes,
                   uint64_t seed, uint64_t epoch, int pad, bool flip, bool train, hipStream_t st) {
  if (n <= 0) return;
  dispatch_row_vec(bf16_out, W, [&](auto t, auto v_c) {
    launch<decltype(t), decltype(v_c)::value>(rec, idx, affine, x, y, n, C, H, W, label_bytes,
                                              seed, epoch, pad, flip, train, st);
  });
}

}  // namespace mipipe
