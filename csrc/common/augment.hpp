// Per-sample augmentation of the record loaders: TrivialAugmentWide on the stored uint8 image and
// Random Erasing on the normalised output, shared by the host loader (csrc/runtime/loader.cpp) and
// the device kernels (csrc/kernels/augment.hip).  As in rrc.hpp everything is integer arithmetic
// on (seed, epoch, sample index) and 8-bit pixels — Q16 factors, floor shifts, literal tables, no
// float — so every implementation produces the same bytes (mipipe/data/records.py holds the NumPy
// definition; tests compare the three).
//
// Words of a sample: h0 = sample_word() is the crop / flip word of the two transforms, unchanged;
// a = splitmix64(h0 ^ kAugSalt) drives the augmentation, e = splitmix64(h0 ^ kEraseSalt) the erase.
//
// The op table is laid out for policies of several ops per image (RandAugment, AutoAugment) to
// reuse: an op is (Op, magnitude bin 0..30, sign), its code path is op_kind(), and every path is a
// function of the source image alone, so a second op is a second pass.
#pragma once
#include <cstdint>

#include "rrc.hpp"

#define MIPIPE_AUG_HD MIPIPE_RRC_HD

namespace mipipe_aug {

using mipipe_rrc::isqrt64;
using mipipe_rrc::splitmix64;

constexpr uint64_t kAugSalt = 0x5441776964654f70ull;
constexpr uint64_t kEraseSalt = 0x52616e6445726173ull;
constexpr int kOps = 14;
constexpr int kBins = 31;
constexpr int kEraseAttempts = 10;
constexpr int kEraseRatios = 64;

enum Op {
  kIdentity = 0, kShearX, kShearY, kTranslateX, kTranslateY, kRotate, kBrightness, kColor,
  kContrast, kSharpness, kPosterize, kSolarize, kAutoContrast, kEqualize
};

// the four code paths the 14 ops collapse to
enum Kind { kLut = 0, kColorBlend = 1, kStencil = 2, kAffine = 3 };

struct Params {
  int op, m, sign;  // sign: +1 or -1
};

MIPIPE_AUG_HD uint64_t sample_word(uint64_t seed, uint64_t epoch, uint64_t index) {
  return splitmix64(seed ^ splitmix64(epoch * 0x100000001b3ull ^ index));
}

// TrivialAugmentWide: one op, one of 31 magnitude bins, a random sign.  force >= 0 pins them:
// op | m << 8 | (sign is +1) << 16.
MIPIPE_AUG_HD Params ta_wide_params(uint64_t h0, int64_t force) {
  Params p;
  if (force >= 0) {
    p.op = (int)(force & 0xff);
    p.m = (int)((force >> 8) & 0xff);
    p.sign = ((force >> 16) & 1) ? 1 : -1;
    return p;
  }
  const uint64_t a = splitmix64(h0 ^ kAugSalt);
  p.op = (int)(((a & 0xffffffffull) * kOps) >> 32);
  p.m = (int)((((a >> 32) & 0xffffffull) * kBins) >> 24);
  p.sign = ((a >> 60) & 1) ? 1 : -1;
  return p;
}

MIPIPE_AUG_HD bool force_ok(int64_t force) {
  return force < 0 || (force < (1 << 17) && (force & 0xff) < kOps && ((force >> 8) & 0xff) < kBins);
}

MIPIPE_AUG_HD int op_kind(int op, int C) {
  if (op >= kShearX && op <= kRotate) return kAffine;
  if (op == kColor) return C == 3 ? kColorBlend : kLut;  // one channel: the identity table
  if (op == kSharpness) return kStencil;
  return kLut;
}

// 0.99 * m / 30 in Q16 and the enhancement factor 1 + sign * that
MIPIPE_AUG_HD int mag_q16(int m) { return (64881 * m) / 30; }
MIPIPE_AUG_HD int factor_q16(const Params& p) { return 65536 + p.sign * mag_q16(p.m); }

// (d * (1 - f) + v * f) rounded and clamped: d, v in [0, 255], fq in [655, 130417], so the sum
// stays inside 32 bits.  The sum is clamped to [0, 2^24) before the floor shift, which gives the
// clamp of the shifted value to [0, 255]; in the other order hipcc 7 packs two such results with
// v_ashr_pk_u8_i32 for gfx950 and then reads the register's upper half, which that instruction
// leaves as it was.
MIPIPE_AUG_HD int blend(int d, int v, int fq) {
  const int s = d * (65536 - fq) + v * fq + 32768;
  return (s < 0 ? 0 : (s > 0xffffff ? 0xffffff : s)) >> 16;
}

MIPIPE_AUG_HD int grey(int r, int g, int b) {
  return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}

// table entry of the ops that are a function of the pixel alone; `mean` is Contrast's image mean
MIPIPE_AUG_HD int point_lut(const Params& p, int mean, int v) {
  switch (p.op) {
    case kBrightness: return blend(0, v, factor_q16(p));
    case kContrast: return blend(mean, v, factor_q16(p));
    case kPosterize: {
      const int bits = 8 - (2 * p.m + 5) / 10;
      return v & ((0xff << (8 - bits)) & 0xff);
    }
    case kSolarize: return 2 * v < 510 - 17 * p.m ? v : 255 - v;
    default: return v;
  }
}

// Contrast's mean from the sum of the grey values of npix pixels
MIPIPE_AUG_HD int contrast_mean(uint64_t grey_sum, uint64_t npix) {
  return (int)((2 * grey_sum + npix) / (2 * npix));
}

// AutoContrast / Equalize: the 256-entry table of one channel from its histogram
template <class H, class L>
MIPIPE_AUG_HD void hist_lut(int op, const H* hist, L* lut) {
  int lo = 256, hi = -1, nonzero = 0;
  uint64_t total = 0;
  for (int i = 0; i < 256; ++i) {
    if (hist[i]) {
      if (lo == 256) lo = i;
      hi = i;
      ++nonzero;
      total += hist[i];
    }
  }
  if (op == kAutoContrast) {
    for (int i = 0; i < 256; ++i) {
      int v = i;
      if (hi > lo) {  // values outside [lo, hi] do not occur
        v = ((i - lo) * 255) / (hi - lo);
        v = i < lo ? 0 : (v > 255 ? 255 : v);
      }
      lut[i] = (L)v;
    }
    return;
  }
  const uint64_t step = nonzero >= 2 ? (total - hist[hi]) / 255 : 0;
  uint64_t cum = 0;
  for (int i = 0; i < 256; ++i) {
    uint64_t v = (uint64_t)i;
    if (step) {
      v = (step / 2 + cum) / step;
      if (v > 255) v = 255;
    }
    lut[i] = (L)v;
    cum += hist[i];
  }
}

// round(65536 * cos / sin(4.5 deg * m)): Rotate's 31 angles, 0 .. 135 degrees
MIPIPE_AUG_HD int cos_q16(int m) {
  constexpr int kCos[kBins] = {65536,  65334,  64729,  63725,  62328,  60547,  58393,  55879,
                               53020,  49834,  46341,  42562,  38521,  34242,  29753,  25080,
                               20252,  15299,  10252,  5142,   0,      -5142,  -10252, -15299,
                               -20252, -25080, -29753, -34242, -38521, -42562, -46341};
  return kCos[m];
}
MIPIPE_AUG_HD int sin_q16(int m) {
  constexpr int kSin[kBins] = {0,     5142,  10252, 15299, 20252, 25080, 29753, 34242,
                               38521, 42562, 46341, 49834, 53020, 55879, 58393, 60547,
                               62328, 63725, 64729, 65334, 65536, 65334, 64729, 63725,
                               62328, 60547, 58393, 55879, 53020, 49834, 46341};
  return kSin[m];
}

// The inverse map of the geometric ops in doubled centred coordinates (u = 2x + 1 - W,
// v = 2y + 1 - H): su = ((A u + B v) >> 16) + 2 tx, sv = ((C u + D v) >> 16) + 2 ty.
struct Affine {
  int A, B, C, D, tx, ty;
};

MIPIPE_AUG_HD Affine affine_of(const Params& p) {
  Affine a{65536, 0, 0, 65536, 0, 0};
  const int sq = p.sign * mag_q16(p.m);
  switch (p.op) {
    case kShearX: a.B = -sq; break;
    case kShearY: a.C = -sq; break;
    case kTranslateX: a.tx = -p.sign * ((32 * p.m) / 30); break;
    case kTranslateY: a.ty = -p.sign * ((32 * p.m) / 30); break;
    case kRotate:
      a.A = a.D = cos_q16(p.m);
      a.B = p.sign * sin_q16(p.m);
      a.C = -p.sign * sin_q16(p.m);
      break;
    default: break;
  }
  return a;
}

// source pixel of output (y, x), nearest neighbour; false: outside the image (the result is 0)
MIPIPE_AUG_HD bool affine_src(const Affine& a, int y, int x, int H, int W, int* ys, int* xs) {
  const int64_t u = 2 * (int64_t)x + 1 - W, v = 2 * (int64_t)y + 1 - H;
  const int64_t su = ((a.A * u + a.B * v) >> 16) + 2 * a.tx;
  const int64_t sv = ((a.C * u + a.D * v) >> 16) + 2 * a.ty;
  const int64_t sx = (su + W) >> 1, sy = (sv + H) >> 1;
  if (sx < 0 || sx >= W || sy < 0 || sy >= H) return false;
  *xs = (int)sx;
  *ys = (int)sy;
  return true;
}

// Sharpness at (y, x) of a plane: the blend of the pixel with the 3x3 smoothing (centre weight 5,
// sum 13) on interior pixels; border pixels keep their value
MIPIPE_AUG_HD int sharpen(const uint8_t* plane, int y, int x, int H, int W, int fq) {
  const uint8_t* p = plane + (int64_t)y * W + x;
  const int v = p[0];
  if (y < 1 || x < 1 || y >= H - 1 || x >= W - 1) return v;
  const int acc = p[-W - 1] + p[-W] + p[-W + 1] + p[-1] + 5 * v + p[1] + p[W - 1] + p[W] + p[W + 1];
  return blend((acc + 6) / 13, v, fq);
}

// ------------------------------------------------------------------------------ Random Erasing
// round(65536 * 0.3 * 11^(t/63)): aspect ratios h/w, log-uniform over [0.3, 1/0.3]
MIPIPE_AUG_HD uint32_t erase_ratio_q16(int t) {
  constexpr uint32_t kRatio[kEraseRatios] = {
      19661,  20424,  21216,  22039,  22894,  23782,  24705,  25663,  26659,  27693,  28767,
      29884,  31043,  32247,  33498,  34798,  36148,  37550,  39007,  40520,  42092,  43725,
      45422,  47184,  49014,  50916,  52891,  54943,  57075,  59289,  61589,  63978,  66460,
      69039,  71717,  74499,  77390,  80392,  83511,  86751,  90116,  93612,  97244,  101017,
      104936, 109007, 113236, 117629, 122192, 126933, 131857, 136972, 142286, 147806, 153541,
      159497, 165685, 172113, 178790, 185726, 192932, 200417, 208192, 216269};
  return kRatio[t];
}

struct EraseBox {
  int y0, x0, h, w;  // h == 0: nothing is erased
  int attempt;       // the accepted attempt; -1: not applied, -2: all ten rejected
};

// torchvision RandomErasing.get_params (scale 0.02-0.33, ratio 0.3-3.3) on an Ho x Wo output,
// applied iff the low 24 bits of the erase word are below pq = round(p * 2^24).  Ho, Wo <= 32768.
MIPIPE_AUG_HD EraseBox erase_box(uint64_t h0, uint32_t pq, int Ho, int Wo) {
  EraseBox b{0, 0, 0, 0, -1};
  const uint64_t e = splitmix64(h0 ^ kEraseSalt);
  if ((e & 0xffffffull) >= pq) return b;
  for (int k = 0; k < kEraseAttempts; ++k) {
    const uint64_t g = splitmix64(e + (uint64_t)k + 1);
    const uint64_t sq = 1311 + (((21627 - 1311) * (g & 0xffffffull)) >> 24);
    const uint64_t area = ((uint64_t)Ho * Wo * sq) >> 16;
    const uint64_t r = erase_ratio_q16((int)((g >> 24) & (kEraseRatios - 1)));
    const uint64_t h = isqrt64((area * r) >> 16);
    const uint64_t w = isqrt64((area << 16) / r);
    if (h > 0 && h < (uint64_t)Ho && w > 0 && w < (uint64_t)Wo) {
      const uint64_t g2 = splitmix64(g);
      b.h = (int)h;
      b.w = (int)w;
      b.y0 = (int)((g2 & 0xffffffffull) % (uint64_t)(Ho - b.h + 1));
      b.x0 = (int)((g2 >> 32) % (uint64_t)(Wo - b.w + 1));
      b.attempt = k;
      return b;
    }
  }
  b.attempt = -2;
  return b;
}

}  // namespace mipipe_aug
