// Launchers of dwconv7.hip: the ConvNeXt block's 7x7 depthwise convolution and its closing
// layer scale + stochastic depth + residual.  The bindings (bind/convnext.cpp) check every
// argument and allocate outputs and workspaces; the launchers neither allocate nor synchronise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mipipe {

// ---- depthwise 7x7, stride 1, pad 3, NHWC, C % 8 == 0 --------------------------------------------
// A block computes a kDw7TileH x kDw7TileW output tile of one channel block (kDw7ChanBytes of
// channels: 64 bf16 / 32 fp32) from an LDS halo patch filled once.
constexpr int kDw7TileH = 8;
constexpr int kDw7TileW = 16;
constexpr int kDw7ChanBytes = 128;
constexpr int kDw7MaxChannels = 2048;
constexpr int kDw7MaxBlocks = 4096;  // spatial blocks per channel block (grid-strided beyond)
// weight-grad: P partial rows (= spatial blocks per channel block), P * channel blocks aimed at
// kDw7WgradBlocks, P in [kDw7WgradMinRows, kDw7WgradMaxRows] and at most the number of tiles
constexpr int kDw7WgradBlocks = 1024;
constexpr int kDw7WgradMinRows = 16;
constexpr int kDw7WgradMaxRows = 512;

inline int dw7_chan_block(bool f32) { return kDw7ChanBytes / (f32 ? 4 : 2); }
inline long dw7_tiles(int N, int H, int W) {
  return (long)N * ((H + kDw7TileH - 1) / kDw7TileH) * ((W + kDw7TileW - 1) / kDw7TileW);
}
inline int dw7_wgrad_rows(int N, int H, int W, int C, bool f32) {
  const int cb = dw7_chan_block(f32);
  const int ncb = (C + cb - 1) / cb;
  long p = kDw7WgradBlocks / ncb;
  if (p < kDw7WgradMinRows) p = kDw7WgradMinRows;
  if (p > kDw7WgradMaxRows) p = kDw7WgradMaxRows;
  const long t = dw7_tiles(N, H, W);
  return (int)(p < t ? p : t);
}

// y = T(bias[c] + sum_taps x * w) (+ addend, in fp32 before the rounding).  w: [C, 7, 7, 1] in T.
// flip: the taps mirrored (the data-grad: x = dy, y = dx).  bias / addend may be null.
void dwconv7_fwd(const void* x, const void* w, const float* bias, const void* addend, void* y,
                 int N, int H, int W, int C, bool flip, bool f32, hipStream_t st);
// dw [C, 49] += sum dy * x(shifted), db [C] += sum dy, through ws_w [P, C*49] / ws_b [P, C]
// partial rows (P = dw7_wgrad_rows) summed in a fixed order: no atomics.
void dwconv7_wgrad(const void* dy, const void* x, float* ws_w, float* ws_b, float* dw, float* db,
                   int N, int H, int W, int C, bool f32, hipStream_t st);

// ---- layer scale + stochastic depth ("row" mode) + residual --------------------------------------
// rows R = N * HW, sample n = r / HW, s_n = keep(n) ? scale : 0 with keep the dropout hash of the
// sample index (thr == 0: always kept).
struct PathDrop {
  float scale;  // fp32(1 / (1 - p)), 1 when p == 0
  uint32_t thr, seed;
  const uint32_t* seed_dev;
};
// p * 2^32 as the hash threshold, as the dropout launchers compute it
inline uint32_t drop_threshold_host(double p) {
  const double t = p * 4294967296.0;
  return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}
// forward: a block streams tiles of kSrFwdThreads * kSrFwdItems 8-channel items, grid-strided past
// kSrFwdMaxBlocks blocks
constexpr int kSrFwdThreads = 256;
constexpr int kSrFwdItems = 4;
constexpr int kSrFwdMaxBlocks = 2048;
constexpr int kSrBlockRows = 128;  // rows a backward block takes per pass (32 row lanes x 4)
constexpr int kSrMaxBlocks = 1024;
inline int sr_bwd_rows(long R, int C) {
  const int ncc = (C + 63) / 64;
  long p = (R + kSrBlockRows - 1) / kSrBlockRows;
  const long cap = kSrMaxBlocks / ncc > 1 ? kSrMaxBlocks / ncc : 1;
  return (int)(p < cap ? (p < 1 ? 1 : p) : cap);
}
// out = T(res + (f * gamma[c]) * s_n): three rounded fp32 operations
void scale_residual_fwd(const void* f, const void* res, const float* gamma, void* out, long R,
                        int C, int HW, PathDrop d, bool f32, hipStream_t st);
// df = T((dout * gamma[c]) * s_n); dgamma[c] += sum_r (dout * f) * s_n; dbias[c] += sum_r df
// (dbias / ws_b null: not wanted).  ws_g / ws_b: [sr_bwd_rows, C] partial rows.
void scale_residual_bwd(const void* dout, const void* f, const float* gamma, void* df, float* ws_g,
                        float* ws_b, float* dgamma, float* dbias, long R, int C, int HW,
                        PathDrop d, bool f32, hipStream_t st);

}  // namespace mipipe
