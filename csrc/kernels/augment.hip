// Per-sample augmentation on the device (the host side is RecordLoader::augmented / erase in
// csrc/runtime/loader.cpp; the definitions are csrc/common/augment.hpp, integer-only, so both
// sides give the same bytes).
//
// record_augment: TrivialAugmentWide on whole uint8 records, out of place (the gathers cannot run
// in place): rec [n][label_bytes + C*H*W] -> out of the same layout, label bytes copied; the decode
// kernels of records.hip then read `out` as they read `rec`.  A work unit is (sample, part): thread
// 0 derives (op, magnitude, sign) from (seed, epoch, idx[s]) — or from `force` — and the block
// takes one of four paths:
//   table   : a 256-entry byte table per channel in LDS (Identity, Brightness, Contrast, Posterize,
//             Solarize, AutoContrast, Equalize, and Color on one channel).  Contrast first sums the
//             grey values of the sample (64-bit LDS integer atomics), AutoContrast / Equalize first
//             build the channels' histograms (32-bit LDS integer atomics); every block that works
//             on such a sample redoes that pass (re-reads come from L2), so at most two blocks
//             share it.
//   colour  : the blend of each pixel with its grey value (three channels)
//   stencil : Sharpness, a 3x3 smoothing blended with the pixel, borders kept
//   affine  : ShearX/Y, TranslateX/Y, Rotate as one inverse nearest-neighbour gather, fill 0
// Nothing in a record is aligned (3x256x256 with 2 label bytes: a stride of 196,610 bytes), so the
// image of a sample is written as [bytes up to the first 4-byte boundary of the destination |
// 32-bit words | tail bytes]; the table path also reads words when source and destination share
// their alignment modulo 4, the reductions read four bytes at a time through memcpy (the compiler
// picks a load that is legal at any alignment), everything else reads bytes.
//
// batch_erase: Random Erasing in place on the decoded NCHW batch (fp32 or bf16: zero is the
// all-zero word in both).  A work unit is (sample, slice): thread 0 derives the box from (seed,
// epoch, idx[s], pq, Ho, Wo); a sample that is not erased touches no memory; the C * h rows of the
// box are zeroed as [elements up to the first 16-byte boundary | 16-byte stores | tail elements].
#include "../common/augment.hpp"
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

namespace aug = mipipe_aug;

constexpr int kAugThreads = 256;
constexpr int kReduceParts = 2;

struct AugGeom {
  int C, H, W;
  uint32_t plane, per;
  FastDiv fW, fPlane;
};

// (channel, row, column) of flat image offset e; next() steps to e + 1
struct AugPos {
  uint32_t c, y, x;
  __device__ __forceinline__ AugPos(const AugGeom& g, uint32_t e) {
    c = g.fPlane.div(e);
    const uint32_t r = e - c * g.plane;
    y = g.fW.div(r);
    x = r - y * (uint32_t)g.W;
  }
  __device__ __forceinline__ void next(const AugGeom& g) {
    if (++x == (uint32_t)g.W) {
      x = 0;
      if (++y == (uint32_t)g.H) {
        y = 0;
        ++c;
      }
    }
  }
};

// the paths that work on (c, y, x): one division pair per word, the other three bytes by stepping
template <class P>
struct ByPos : P {
  __device__ __forceinline__ ByPos(const P& p) : P(p) {}
  __device__ __forceinline__ uint32_t at(uint32_t e) const { return P::at(AugPos(this->g, e)); }
  __device__ __forceinline__ uint32_t at4(uint32_t e) const {
    AugPos p(this->g, e);
    uint32_t w = P::at(p);
    p.next(this->g);
    w |= P::at(p) << 8;
    p.next(this->g);
    w |= P::at(p) << 16;
    p.next(this->g);
    return w | P::at(p) << 24;
  }
};

__device__ __forceinline__ uint32_t load4(const uint8_t* p) {  // any alignment
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// One byte of the result at flat image offset e, per path ------------------------------------
struct TablePath {
  const uint8_t* lut;  // LDS, [C][256]
  const uint8_t* src;
  uint32_t plane;
  bool words;  // src + e is 4-byte aligned wherever dst + e is
  __device__ __forceinline__ uint32_t chan(uint32_t e) const {
    return (uint32_t)(e >= plane) + (uint32_t)(e >= 2 * plane);
  }
  __device__ __forceinline__ uint32_t at(uint32_t e) const { return lut[chan(e) * 256 + src[e]]; }
  __device__ __forceinline__ uint32_t at4(uint32_t e) const {
    if (!words) return at(e) | at(e + 1) << 8 | at(e + 2) << 16 | at(e + 3) << 24;
    const uint32_t v = *reinterpret_cast<const uint32_t*>(src + e);
    return (uint32_t)lut[chan(e) * 256 + (v & 0xff)] |
           (uint32_t)lut[chan(e + 1) * 256 + ((v >> 8) & 0xff)] << 8 |
           (uint32_t)lut[chan(e + 2) * 256 + ((v >> 16) & 0xff)] << 16 |
           (uint32_t)lut[chan(e + 3) * 256 + (v >> 24)] << 24;
  }
};

struct ColourPath {
  const uint8_t* src;
  uint32_t plane;
  int fq;
  __device__ __forceinline__ uint32_t at(uint32_t e) const {
    const uint32_t c = (uint32_t)(e >= plane) + (uint32_t)(e >= 2 * plane);
    const uint32_t p = e - c * plane;
    const int g = aug::grey(src[p], src[plane + p], src[2 * plane + p]);
    return (uint32_t)aug::blend(g, src[e], fq);
  }
  __device__ __forceinline__ uint32_t at4(uint32_t e) const {
    return at(e) | at(e + 1) << 8 | at(e + 2) << 16 | at(e + 3) << 24;
  }
};

struct StencilPath {
  const uint8_t* src;
  AugGeom g;
  int fq;
  __device__ __forceinline__ uint32_t at(const AugPos& p) const {
    return (uint32_t)aug::sharpen(src + (size_t)p.c * g.plane, (int)p.y, (int)p.x, g.H, g.W, fq);
  }
};

struct AffinePath {
  const uint8_t* src;
  AugGeom g;
  aug::Affine a;
  __device__ __forceinline__ uint32_t at(const AugPos& p) const {
    int ys, xs;
    if (!aug::affine_src(a, (int)p.y, (int)p.x, g.H, g.W, &ys, &xs)) return 0;
    return src[(size_t)p.c * g.plane + (size_t)ys * g.W + xs];
  }
};

// this part's share of the sample's `per` result bytes: items [head | words | tail] of dst
template <class P>
__device__ __forceinline__ void write_image(const P& path, uint8_t* dst, uint32_t per, int part,
                                            int parts) {
  const uint32_t head = min(per, (uint32_t)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3));
  const uint32_t nw = (per - head) / 4;
  const uint32_t items = nw + 2;
  for (uint32_t it = (uint32_t)part * kAugThreads + threadIdx.x; it < items;
       it += (uint32_t)parts * kAugThreads) {
    if (it >= 1 && it <= nw) {
      const uint32_t e = head + (it - 1) * 4;
      *reinterpret_cast<uint32_t*>(dst + e) = path.at4(e);
    } else {
      const uint32_t b0 = it == 0 ? 0 : head + nw * 4;
      const uint32_t b1 = it == 0 ? head : per;
      for (uint32_t e = b0; e < b1; ++e) dst[e] = (uint8_t)path.at(e);
    }
  }
}

__global__ __launch_bounds__(kAugThreads) void record_augment_kernel(
    const uint8_t* __restrict__ rec, const int64_t* __restrict__ idx, uint8_t* __restrict__ out,
    long n, AugGeom g, int label_bytes, long rec_bytes, uint64_t seed, uint64_t epoch,
    long force, int parts) {
  __shared__ aug::Params s_par;
  __shared__ unsigned long long s_sum;
  __shared__ uint32_t s_hist[3 * 256];
  __shared__ __attribute__((aligned(4))) uint8_t s_lut[3 * 256];
  const long units = n * parts;
  const int tid = (int)threadIdx.x;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long s = u / parts;
    const int part = (int)(u - s * parts);
    const uint8_t* r = rec + s * rec_bytes;
    uint8_t* o = out + s * rec_bytes;
    if (tid == 0) {
      s_par = aug::ta_wide_params(aug::sample_word(seed, epoch, (uint64_t)idx[s]), force);
      s_sum = 0;
      if (part == 0)
        for (int k = 0; k < label_bytes; ++k) o[k] = r[k];
    }
    for (int t = tid; t < 3 * 256; t += kAugThreads) s_hist[t] = 0;
    __syncthreads();
    const aug::Params par = s_par;
    const uint8_t* img = r + label_bytes;
    uint8_t* dst = o + label_bytes;
    const int kind = aug::op_kind(par.op, g.C);
    int nparts = parts;  // blocks that share this sample
    if (kind == aug::kLut) {
      // The reduction the table needs runs over the whole sample in every block that works on it
      // (re-reads come from L2).  The LDS atomics of the histograms are the expensive part, so a
      // sample with a reduction is shared by at most kReduceParts blocks; the others skip it.
      const bool hist = par.op == aug::kAutoContrast || par.op == aug::kEqualize;
      if (hist || par.op == aug::kContrast) {
        nparts = min(parts, kReduceParts);
        if (part >= nparts) {
          __syncthreads();
          continue;
        }
      }
      if (par.op == aug::kContrast) {
        unsigned long long acc = 0;
        const uint32_t nw = g.plane / 4;
        for (uint32_t i = (uint32_t)tid; i < nw; i += kAugThreads) {
          const uint32_t r = load4(img + 4 * i);
          const uint32_t gg = g.C == 3 ? load4(img + g.plane + 4 * i) : 0;
          const uint32_t b = g.C == 3 ? load4(img + 2 * g.plane + 4 * i) : 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int rj = (int)((r >> (8 * j)) & 0xff);
            acc += (unsigned)(g.C == 3 ? aug::grey(rj, (int)((gg >> (8 * j)) & 0xff),
                                                   (int)((b >> (8 * j)) & 0xff))
                                       : rj);
          }
        }
        for (uint32_t p = nw * 4 + (uint32_t)tid; p < g.plane; p += kAugThreads)
          acc += (unsigned)(g.C == 3 ? aug::grey(img[p], img[g.plane + p], img[2 * g.plane + p])
                                     : (int)img[p]);
        atomicAdd(&s_sum, acc);
      } else if (hist) {
        const uint32_t nw = g.per / 4;
        for (uint32_t i = (uint32_t)tid; i < nw; i += kAugThreads) {
          const uint32_t v = load4(img + 4 * i);
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t e = 4 * i + j;
            const uint32_t c = (uint32_t)(e >= g.plane) + (uint32_t)(e >= 2 * g.plane);
            atomicAdd(&s_hist[c * 256 + ((v >> (8 * j)) & 0xff)], 1u);
          }
        }
        for (uint32_t e = nw * 4 + (uint32_t)tid; e < g.per; e += kAugThreads) {
          const uint32_t c = (uint32_t)(e >= g.plane) + (uint32_t)(e >= 2 * g.plane);
          atomicAdd(&s_hist[c * 256 + img[e]], 1u);
        }
      }
      __syncthreads();
      if (par.op == aug::kAutoContrast || par.op == aug::kEqualize) {
        if (tid < g.C) aug::hist_lut(par.op, s_hist + tid * 256, s_lut + tid * 256);
      } else {
        const int mean = par.op == aug::kContrast ? aug::contrast_mean(s_sum, g.plane) : 0;
        const uint8_t v = (uint8_t)aug::point_lut(par, mean, tid);  // kAugThreads == 256
        for (int c = 0; c < g.C; ++c) s_lut[c * 256 + tid] = v;
      }
      __syncthreads();
      TablePath path{s_lut, img, g.plane,
                     ((reinterpret_cast<uintptr_t>(img) ^ reinterpret_cast<uintptr_t>(dst)) & 3) == 0};
      write_image(path, dst, g.per, part, nparts);
    } else if (kind == aug::kColorBlend) {
      write_image(ColourPath{img, g.plane, aug::factor_q16(par)}, dst, g.per, part, parts);
    } else if (kind == aug::kStencil) {
      write_image(ByPos<StencilPath>(StencilPath{img, g, aug::factor_q16(par)}), dst, g.per, part,
                  parts);
    } else {
      write_image(ByPos<AffinePath>(AffinePath{img, g, aug::affine_of(par)}), dst, g.per, part,
                  parts);
    }
    __syncthreads();  // s_par, s_sum, s_hist and s_lut are rewritten by the next unit
  }
}

// ------------------------------------------------------------------------------- batch_erase
constexpr int kEraseThreads = 256;

template <class U>  // the element as an unsigned word: uint32_t (fp32) or uint16_t (bf16)
__global__ __launch_bounds__(kEraseThreads) void batch_erase_kernel(
    U* __restrict__ x, const int64_t* __restrict__ idx, long n, int C, int Ho, int Wo,
    uint64_t seed, uint64_t epoch, uint32_t pq, int slices) {
  constexpr uint32_t V = 16 / sizeof(U);
  __shared__ aug::EraseBox s_box;
  const long per = (long)C * Ho * Wo;
  const long units = n * slices;
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long s = u / slices;
    const int slice = (int)(u - s * slices);
    if (threadIdx.x == 0)
      s_box = aug::erase_box(aug::sample_word(seed, epoch, (uint64_t)idx[s]), pq, Ho, Wo);
    __syncthreads();
    const aug::EraseBox b = s_box;
    __syncthreads();  // s_box is rewritten by the next unit
    if (b.h <= 0 || b.w <= 0) continue;  // not erased: no memory is touched
    U* xs = x + s * per;
    const uint32_t L = (uint32_t)b.w;
    const uint32_t ipr = L / V + 2;  // items of a row: [head | 16-byte vectors | tail]
    const uint32_t items = (uint32_t)C * (uint32_t)b.h * ipr;  // <= per + 2 C Ho < 2^32
    for (uint32_t it = (uint32_t)slice * kEraseThreads + threadIdx.x; it < items;
         it += (uint32_t)slices * kEraseThreads) {
      const uint32_t row = it / ipr;  // c * h + r
      const uint32_t k = it - row * ipr;
      const uint32_t c = row / (uint32_t)b.h;
      const uint32_t y = (uint32_t)b.y0 + row - c * (uint32_t)b.h;
      U* p = xs + ((size_t)c * Ho + y) * Wo + b.x0;
      const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(p) & 15) / sizeof(U));
      const uint32_t head = min(L, (V - mis) % V);
      const uint32_t nvec = (L - head) / V;
      if (k >= 1 && k <= nvec) {
        *reinterpret_cast<uint4*>(p + head + (k - 1) * V) = make_uint4(0, 0, 0, 0);
      } else if (k == 0 || k == nvec + 1) {
        const uint32_t b0 = k == 0 ? 0 : head + nvec * V;
        const uint32_t b1 = k == 0 ? head : L;
        for (uint32_t q = b0; q < b1; ++q) p[q] = (U)0;
      }
    }
  }
}

}  // namespace

int record_augment_parts(int C, int H, int W) {
  // a sample of the workload's size (3x256x256) is split over 8 blocks: one block per sample
  // leaves the pass latency-bound at batch sizes near the CU count
  const long per = (long)C * H * W;
  return (int)std::max<long>(1, std::min<long>(8, per / 16384));
}

void record_augment(const uint8_t* rec, const int64_t* idx, uint8_t* out, long n, int C, int H,
                    int W, int label_bytes, uint64_t seed, uint64_t epoch, long force, int parts,
                    hipStream_t st) {
  if (n <= 0) return;
  AugGeom g;
  g.C = C;
  g.H = H;
  g.W = W;
  g.plane = (uint32_t)H * (uint32_t)W;
  g.per = g.plane * (uint32_t)C;
  g.fW = FastDiv((uint32_t)W);
  g.fPlane = FastDiv(g.plane);
  if (parts <= 0) parts = record_augment_parts(C, H, W);
  const long units = n * parts;
  const unsigned grid = (unsigned)std::min<long>(units, 1l << 20);
  const long rec_bytes = (long)label_bytes + (long)g.per;
  hipLaunchKernelGGL(record_augment_kernel, dim3(grid), dim3(kAugThreads), 0, st, rec, idx, out, n,
                     g, label_bytes, rec_bytes, seed, epoch, force, parts);
}

void batch_erase(void* x, bool f32, const int64_t* idx, long n, int C, int Ho, int Wo,
                 uint64_t seed, uint64_t epoch, uint32_t pq, hipStream_t st) {
  if (n <= 0 || pq == 0) return;
  const long bytes = (long)C * Ho * Wo * (f32 ? 4 : 2);
  // the box is at most a third of the sample
  const int slices = (int)std::max<long>(1, std::min<long>(8, bytes / 65536));
  const unsigned grid = (unsigned)std::min<long>(n * slices, 1l << 20);
  if (f32)
    hipLaunchKernelGGL(batch_erase_kernel<uint32_t>, dim3(grid), dim3(kEraseThreads), 0, st,
                       (uint32_t*)x, idx, n, C, Ho, Wo, seed, epoch, pq, slices);
  else
    hipLaunchKernelGGL(batch_erase_kernel<uint16_t>, dim3(grid), dim3(kEraseThreads), 0, st,
                       (uint16_t*)x, idx, n, C, Ho, Wo, seed, epoch, pq, slices);
}

}  // namespace mipipe
