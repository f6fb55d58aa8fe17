// The "rrc" record transform's geometry, shared by the host loader (csrc/runtime/loader.cpp) and
// the device decode (csrc/kernels/records.hip): RandomResizedCrop(scale 0.08-1, ratio 3/4-4/3,
// bilinear, no antialias) + RandomHorizontalFlip in training, a centre crop of 7/8 of the short
// side in evaluation.  Everything here is integer arithmetic on (seed, epoch, sample index) —
// no exp / log / sqrt / float division — so the box, the tap indices and the Q16 interpolation
// weights are the same numbers on every implementation (mipipe/data/records.py holds the NumPy
// definition; tests compare the three).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MIPIPE_RRC_HD __host__ __device__ inline
#else
#define MIPIPE_RRC_HD inline
#endif

namespace mipipe_rrc {

constexpr int kRatios = 64;
constexpr int kAttempts = 10;
constexpr uint32_t kScaleLoQ16 = 5243;  // 0.08 in Q16

struct Box {
  int y0, x0, h, w, flip;
};

// one bilinear tap pair along an axis: source offsets i0 <= i1 inside the box and the Q16 weight
// of i1 (the weight of i0 is 65536 - frac)
struct Tap {
  int i0, i1;
  uint32_t frac;
};

MIPIPE_RRC_HD uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// round(65536 * 0.75 * (16/9)^(t/63)): aspect ratios w/h, log-uniform over [3/4, 4/3]
MIPIPE_RRC_HD uint32_t ratio_q16(int t) {
  constexpr uint32_t kRatioQ16[kRatios] = {
      49152, 49603, 50058, 50517, 50981, 51449, 51921, 52397, 52878, 53363, 53852, 54346, 54845,
      55348, 55856, 56368, 56886, 57407, 57934, 58466, 59002, 59543, 60090, 60641, 61197, 61759,
      62325, 62897, 63474, 64057, 64644, 65237, 65836, 66440, 67050, 67665, 68285, 68912, 69544,
      70182, 70826, 71476, 72132, 72793, 73461, 74135, 74815, 75502, 76195, 76894, 77599, 78311,
      79030, 79755, 80486, 81225, 81970, 82722, 83481, 84247, 85020, 85800, 86587, 87381};
  return kRatioQ16[t];
}

// floor(sqrt(v)), bit by bit
MIPIPE_RRC_HD uint64_t isqrt64(uint64_t v) {
  uint64_t r = 0, bit = 1ull << 62;
  while (bit > v) bit >>= 2;
  while (bit) {
    if (v >= r + bit) {
      v -= r + bit;
      r = (r >> 1) + bit;
    } else {
      r >>= 1;
    }
    bit >>= 2;
  }
  return r;
}

// The source box of sample `index`.  H, W <= 32768 (the callers check), so every product fits.
MIPIPE_RRC_HD Box rrc_box(uint64_t seed, uint64_t epoch, uint64_t index, int H, int W, bool train,
                          bool flip_enabled) {
  Box b;
  if (!train) {
    const int s = ((H < W ? H : W) * 7) / 8;
    b.y0 = (H - s) / 2;
    b.x0 = (W - s) / 2;
    b.h = b.w = s;
    b.flip = 0;
    return b;
  }
  const uint64_t h0 = splitmix64(seed ^ splitmix64(epoch * 0x100000001b3ull ^ index));
  b.flip = flip_enabled && ((h0 >> 40) & 1);
  for (int k = 0; k < kAttempts; ++k) {
    const uint64_t g = splitmix64(h0 + (uint64_t)k + 1);
    const uint64_t sq = kScaleLoQ16 + (((65536 - kScaleLoQ16) * (g & 0xffffff)) >> 24);
    const uint64_t area = ((uint64_t)H * W * sq) >> 16;
    const uint64_t r = ratio_q16((int)((g >> 24) & (kRatios - 1)));
    const uint64_t w = isqrt64((area * r) >> 16);
    const uint64_t h = isqrt64((area << 16) / r);
    if (w > 0 && w <= (uint64_t)W && h > 0 && h <= (uint64_t)H) {
      const uint64_t g2 = splitmix64(g);
      b.h = (int)h;
      b.w = (int)w;
      b.y0 = (int)((g2 & 0xffffffffull) % (uint64_t)(H - b.h + 1));
      b.x0 = (int)((g2 >> 32) % (uint64_t)(W - b.w + 1));
      return b;
    }
  }
  b.h = H;
  b.w = W;
  if (4 * (int64_t)W < 3 * (int64_t)H) b.h = (4 * W) / 3;
  else if (3 * (int64_t)W > 4 * (int64_t)H) b.w = (4 * H) / 3;
  b.y0 = (H - b.h) / 2;
  b.x0 = (W - b.w) / 2;
  return b;
}

// taps of output coordinate o on an axis resampled from n_in to n_out (half-pixel centres,
// clamped at the edges): p = ((2o+1) * n_in * 2^15) / n_out - 2^15 in Q16, floored.
MIPIPE_RRC_HD Tap rrc_tap(int o, int n_in, int n_out) {
  int64_t p = (int64_t)((((uint64_t)(2 * (int64_t)o + 1) * (uint64_t)n_in) << 15) / (uint64_t)n_out) - 32768;
  if (p < 0) p = 0;
  Tap t;
  t.i0 = (int)(p >> 16);
  t.i1 = t.i0 + 1 < n_in ? t.i0 + 1 : n_in - 1;
  t.frac = (uint32_t)(p & 0xffff);
  return t;
}

}  // namespace mipipe_rrc
