// Depthwise K x K convolution, K in {3, 5}, stride S in {1, 2}, pad (K - 1) / 2, NHWC, no bias
// (EfficientNet's MBConv): forward with BatchNorm's shifted statistics in the same pass,
// data-grad and weight-grad.  T = bf16 | fp32, C % 8 == 0, channel blocks in grid.y (no cap).
//
//   dwconvk_fwd_kernel    A block owns a TH x TW OUTPUT tile of one channel block (128 bytes of
//                         channels).  The ((TH-1)S+K) x ((TW-1)S+K) input halo is filled into LDS
//                         once, every load issued unconditionally from a clamped address and
//                         zeroed by a select outside the image; a thread makes 8 channels x a strip
//                         of SW outputs, walking the strip's (SW-1)S+K input columns once per
//                         filter row.  With STATS a thread also keeps sum (v - shift) and its
//                         square of the values it STORED, over every tile the block walks; the
//                         block adds its threads' sums through LDS in index order into ONE partial
//                         row and det_sum_rows adds the rows: no float atomics, no pass over y.
//   dwconvk_dgrad_kernel  S = 1: the forward loop over dy with the taps mirrored.  S = 2: a block
//                         owns a 16 x 16 tile of dx and fills the 10 x 10 (K = 5; 9 x 9 for K = 3)
//                         dy halo once; a thread owns 8 channels x a 2 x 2 patch of dx, i.e. one
//                         pixel of each parity class, and each class takes only the taps of its
//                         parity (1/2/2/4 for K = 3, 9/6/6/4 for K = 5) as compile-time sets:
//                         every filter tap is used exactly once per patch, no zero-inserted dy, one
//                         owner per dx element; pixels no tap reaches come out as exact zeros.
//   dwconvk_wgrad_kernel  The forward's halo plus the dy tile in LDS; a thread owns 8 channels x
//                         one filter row x a group of tile rows and slides a K-column window of x
//                         along the row (S new columns per output).  Accumulators stay in registers
//                         across all the tiles of the block; the row groups are added through LDS
//                         in index order into one partial row per block, det_sum_rows adds those.
//
// LDS layout of a halo: pixel-major, a pixel = 128 bytes, a row padded to an ODD number of pixels
// (as dwconv7.hip).  The lanes that share a 16-byte LDS read pass differ in the channel group and
// then in the OUTPUT ROW, never in the column.  For S = 1 neighbouring output rows are one halo row
// (an odd number of pixels) apart: conflict-free.  For S = 2 they are two halo rows apart, an even
// number of pixels, whatever the row stride: so the S = 2 halo is folded by ROW parity (even rows
// first, then the odd rows), which puts rows r and r + 2 one folded row apart again.  Folding by
// column parity would not help here (the lanes of a pass share their columns), and it would cut a
// strip's column walk, which visits both parities for every K, into two address streams.
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

constexpr int kDwkThreads = 256;

template <class T, int K, int S>
struct DwK {
  static constexpr int P = (K - 1) / 2;
  static constexpr int KK = K * K;
  static constexpr int TH = 8, TW = S == 1 ? 16 : 8;  // dwk_tile_h / dwk_tile_w
  static constexpr int HR = (TH - 1) * S + K;         // halo rows
  static constexpr int HC = (TW - 1) * S + K;         // halo columns
  static constexpr int HS = HC | 1;                   // halo row stride in pixels (odd)
  static constexpr bool FOLD = S == 2;                // rows by parity: even rows, then odd rows
  static constexpr int HRH = (HR + 1) / 2;
  static constexpr int LROWS = FOLD ? 2 * HRH : HR;
  static constexpr int CB = kDwkChanBytes / (int)sizeof(T);  // channels per block: 64 / 32
  static constexpr int G = CB / 8;                           // 8-channel groups: 8 / 4
  static constexpr int POS = kDwkThreads / G;                // threads per group: 32 / 64
  static constexpr int STRIPS = POS / TH;                    // strips per tile row: 4 / 8
  static constexpr int SW = TW / STRIPS;                     // outputs per strip
  static constexpr int HALO_BYTES = LROWS * HS * kDwkChanBytes;
  static constexpr int W_BYTES = KK * kDwkChanBytes;
  static constexpr int DY_BYTES = TH * TW * kDwkChanBytes;
  static constexpr int STAT_BYTES = 2 * POS * CB * 4;
  static constexpr int FWD_LDS = HALO_BYTES + W_BYTES;
  // weight-grad: thread = (group, filter row kh of KS slots, row group)
  static constexpr int KS = K == 3 ? 4 : 8;
  static constexpr int RG = POS / KS;
  static constexpr int RED_BYTES = RG * G * KK * 8 * 4;
  static constexpr int WGRAD_LDS =
      HALO_BYTES + DY_BYTES > RED_BYTES ? HALO_BYTES + DY_BYTES : RED_BYTES;
  // stride-2 data-grad: DT x DT tile of dx, (DT/2 + 1 + P/2)^2 halo of dy
  static constexpr int DT = kDwkDgradTile;
  static constexpr int DHR = DT / 2 + 1 + P / 2;
  static constexpr int DHS = DHR | 1;
  static constexpr int DGRAD2_LDS = DHR * DHS * kDwkChanBytes + W_BYTES;
  static_assert(TH == 8 && POS % TH == 0 && TW % STRIPS == 0 && SW >= 1, "tile / thread shape");
  static_assert(HS % 2 == 1 && DHS % 2 == 1, "halo row strides must be odd numbers of pixels");
  static_assert(STAT_BYTES <= HALO_BYTES, "the statistics rows reuse the halo");
  static_assert(WGRAD_LDS <= 64 * 1024 && FWD_LDS <= 64 * 1024, "two blocks per CU and more");
  __device__ static __forceinline__ int lrow(int r) {
    return FOLD ? (r & 1) * HRH + (r >> 1) : r;
  }
};

template <class T>
__device__ __forceinline__ Raw8<T> raw_zero() {
  Raw8<T> r;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 2); ++i) r.v[i] = make_uint4(0u, 0u, 0u, 0u);
  return r;
}
template <class T>
__device__ __forceinline__ void lds_put(uint4* base, int group_idx, const Raw8<T>& r) {
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 2); ++i) base[group_idx * (int)(sizeof(T) / 2) + i] = r.v[i];
}
template <class T>
__device__ __forceinline__ void lds_get(const uint4* base, int group_idx, float* f) {
  Raw8<T> r;
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 2); ++i) r.v[i] = base[group_idx * (int)(sizeof(T) / 2) + i];
  unpack_raw(r, f);
}

// The image a patch is read from (IH x IW) and the grid of tiles a block walks (over OH x OW)
struct DwkGeom {
  FastDiv ftw, fth;  // tiles along W, along H
  int N, C;
  int IH, IW;  // the tensor the LDS halo is filled from
  int OH, OW;  // the tensor the tiles cover
  uint32_t ntiles;
};

// Fill ROWS x COLS pixels of the block's channel block into LDS (row stride STRIDE pixels; FOLDH >
// 0: rows by parity, the odd rows FOLDH rows down) from the ih x iw image of sample n with the
// patch's top-left at (h0, w0); outside the image: 0.
template <class T, int ROWS, int COLS, int STRIDE, int FOLDH>
__device__ __forceinline__ void fill_patch(const T* __restrict__ src, uint4* lds, int ih, int iw,
                                           int C, int n, int h0, int w0, int c0) {
  constexpr int G = kDwkChanBytes / (int)sizeof(T) / 8;
  constexpr int kItems = ROWS * COLS * G;
  constexpr int kPer = (kItems + kDwkThreads - 1) / kDwkThreads;
  constexpr int kBatch = 5;
#pragma unroll
  for (int b0 = 0; b0 < kPer; b0 += kBatch) {
    Raw8<T> r[kBatch];
    bool ok[kBatch];
    int dst[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (b0 + k < kPer) {
        const int i = (int)threadIdx.x + (b0 + k) * kDwkThreads;
        const int ic = min(i, kItems - 1);
        const int gi = ic % G, pix = ic / G;
        const int pc = pix % COLS, pr = pix / COLS;
        const int h = h0 + pr, w = w0 + pc, c = c0 + gi * 8;
        ok[k] = h >= 0 && h < ih && w >= 0 && w < iw && c < C;
        const int hc = min(max(h, 0), ih - 1), wc = min(max(w, 0), iw - 1), cc = min(c, C - 8);
        r[k] = ld_raw8(src + (((long)n * ih + hc) * iw + wc) * C + cc);
        const int lr = FOLDH > 0 ? (pr & 1) * FOLDH + (pr >> 1) : pr;
        dst[k] = i < kItems ? (lr * STRIDE + pc) * G + gi : -1;
      }
    }
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (b0 + k < kPer) {
        if (dst[k] >= 0) lds_put<T>(lds, dst[k], ok[k] ? r[k] : raw_zero<T>());
      }
    }
  }
}

// The block's filter rows: channels [c0, c0 + CB) x K*K taps are contiguous in [C, K, K, 1];
// kept in LDS tap-major ([K*K][CB]), mirrored for the stride-1 data-grad.
template <class T, int KK>
__device__ __forceinline__ void fill_filter(const T* __restrict__ w, T* wl, int C, int c0,
                                            bool flip) {
  constexpr int CB = kDwkChanBytes / (int)sizeof(T);
  const int nvalid = min(CB, C - c0) * KK;  // a multiple of 8
  for (int v = threadIdx.x; v < CB * KK / 8; v += kDwkThreads) {
    const int e0 = v * 8;
    float f[8];
    unpack_raw(ld_raw8(w + (long)c0 * KK + min(e0, nvalid - 8)), f);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = e0 + q;
      const int cl = e / KK, tap = e - cl * KK;
      wl[(flip ? KK - 1 - tap : tap) * CB + cl] = from_f32<T>(e0 < nvalid ? f[q] : 0.f);
    }
  }
}

template <int TH, int TW>
__device__ __forceinline__ void tile_pos(const DwkGeom& g, uint32_t tile, int& n, int& h0, int& w0) {
  const uint32_t t = g.ftw.div(tile);
  w0 = (int)(tile - t * g.ftw.d) * TW;
  const uint32_t nn = g.fth.div(t);
  h0 = (int)(t - nn * g.fth.d) * TH;
  n = (int)nn;
}

// ------------------------------------------------ forward, and the stride-1 data-grad (FLIP)
template <class T, int K, int S, bool FLIP, bool ADD, bool STATS>
__device__ __forceinline__ void conv_tiles(const T* __restrict__ x, const T* __restrict__ w,
                                           const float* __restrict__ shift,
                                           const T* __restrict__ addend, T* __restrict__ y,
                                           float* __restrict__ ws_s, float* __restrict__ ws_q,
                                           const DwkGeom& g, char* smem) {
  using D = DwK<T, K, S>;
  uint4* halo = reinterpret_cast<uint4*>(smem);
  const uint4* wlv = reinterpret_cast<const uint4*>(smem + D::HALO_BYTES);
  const int c0 = blockIdx.y * D::CB;
  const int gi = threadIdx.x % D::G, pos = threadIdx.x / D::G;
  const int row = pos % D::TH, strip = pos / D::TH;
  const int c = c0 + gi * 8;

  fill_filter<T, D::KK>(w, reinterpret_cast<T*>(smem + D::HALO_BYTES), g.C, c0, FLIP);
  float sh[8], ssum[8], ssq[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) sh[q] = ssum[q] = ssq[q] = 0.f;
  if constexpr (STATS) ld_f32x8(shift + min(c, g.C - 8), sh);

  for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int n, h0, w0;
    tile_pos<D::TH, D::TW>(g, tile, n, h0, w0);
    __syncthreads();  // the previous tile's reads are done (first pass: nothing pending)
    fill_patch<T, D::HR, D::HC, D::HS, D::FOLD ? D::HRH : 0>(x, halo, g.IH, g.IW, g.C, n,
                                                             h0 * S - D::P, w0 * S - D::P, c0);
    __syncthreads();  // halo and filter are in LDS

    float acc[D::SW][8];
#pragma unroll
    for (int o = 0; o < D::SW; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[o][q] = 0.f;
#pragma unroll 1
    for (int kh = 0; kh < K; ++kh) {
      float wv[K][8];
#pragma unroll
      for (int kw = 0; kw < K; ++kw) lds_get<T>(wlv, (kh * K + kw) * D::G + gi, wv[kw]);
      const int rbase = (D::lrow(row * S + kh) * D::HS + strip * D::SW * S) * D::G + gi;
#pragma unroll
      for (int j = 0; j < (D::SW - 1) * S + K; ++j) {
        float xv[8];
        lds_get<T>(halo, rbase + j * D::G, xv);
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int d = j - kw;
          if (d >= 0 && d % S == 0 && d / S < D::SW) {
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[d / S][q] = fmaf(xv[q], wv[kw][q], acc[d / S][q]);
          }
        }
      }
    }
    const int h = h0 + row, wbase = w0 + strip * D::SW;
    const long rowoff = ((long)n * g.OH + min(h, g.OH - 1)) * g.OW;
    if constexpr (ADD) {
      Raw8<T> a[D::SW];
#pragma unroll
      for (int o = 0; o < D::SW; ++o)
        a[o] = ld_raw8(addend + (rowoff + min(wbase + o, g.OW - 1)) * g.C + min(c, g.C - 8));
#pragma unroll
      for (int o = 0; o < D::SW; ++o) {
        float f[8];
        unpack_raw(a[o], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[o][q] += f[q];
      }
    }
    if (h < g.OH && c < g.C) {
#pragma unroll
      for (int o = 0; o < D::SW; ++o) {
        if (wbase + o < g.OW) {
          store8(y + (rowoff + wbase + o) * g.C + c, acc[o]);
          if constexpr (STATS) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const float v = as_stored<T>(acc[o][q]) - sh[q];
              ssum[q] += v;
              ssq[q] = fmaf(v, v, ssq[q]);
            }
          }
        }
      }
    }
  }
  if constexpr (STATS) {
    // the block's threads, added in position order: red[2][POS][CB]
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      red[pos * D::CB + gi * 8 + q] = ssum[q];
      red[(D::POS + pos) * D::CB + gi * 8 + q] = ssq[q];
    }
    __syncthreads();
    if (threadIdx.x < 2 * D::CB) {
      const int cl = threadIdx.x % D::CB, a = threadIdx.x / D::CB;
      float s = 0.f;
#pragma unroll 8
      for (int k = 0; k < D::POS; ++k) s += red[(a * D::POS + k) * D::CB + cl];
      if (c0 + cl < g.C) (a == 0 ? ws_s : ws_q)[(long)blockIdx.x * g.C + c0 + cl] = s;
    }
  }
}

template <class T, int K, int S, bool STATS>
__global__ __launch_bounds__(kDwkThreads) void dwconvk_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ shift,
    T* __restrict__ y, float* __restrict__ ws_s, float* __restrict__ ws_q, DwkGeom g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv_tiles<T, K, S, false, false, STATS>(x, w, shift, nullptr, y, ws_s, ws_q, g, smem);
}

// ------------------------------------------------------------------------------- data-grad
// S = 2: dx[h, w] = sum over the taps (kh, kw) with (h + P - kh) and (w + P - kw) even of
// dy[(h + P - kh) / 2, (w + P - kw) / 2] * w[kh, kw].  With the tile origin even, the patch pixel
// (2 pr + a, 2 pc + b) takes the taps kh = (a + P) mod 2, ... from the halo rows pr + dr,
// dr = (a + P - kh) / 2 + P / 2 (halo row 0 is dy row h0 / 2 - P / 2), and likewise in w.
template <class T, int K, int S, bool ADD>
__global__ __launch_bounds__(kDwkThreads) void dwconvk_dgrad_kernel(
    const T* __restrict__ dy, const T* __restrict__ w, const T* __restrict__ addend,
    T* __restrict__ dx, DwkGeom g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if constexpr (S == 1) {
    conv_tiles<T, K, 1, true, ADD, false>(dy, w, nullptr, addend, dx, nullptr, nullptr, g, smem);
  } else {
    using D = DwK<T, K, S>;
    constexpr int P = D::P, DT = D::DT;
    constexpr int NW = 2 + P / 2;  // halo rows / columns under a 2 x 2 patch
    constexpr int kHaloBytes = D::DHR * D::DHS * kDwkChanBytes;
    uint4* halo = reinterpret_cast<uint4*>(smem);
    const uint4* wlv = reinterpret_cast<const uint4*>(smem + kHaloBytes);
    const int c0 = blockIdx.y * D::CB;
    fill_filter<T, D::KK>(w, reinterpret_cast<T*>(smem + kHaloBytes), g.C, c0, false);

    for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
      int n, h0, w0;
      tile_pos<DT, DT>(g, tile, n, h0, w0);
      __syncthreads();
      fill_patch<T, D::DHR, D::DHR, D::DHS, 0>(dy, halo, g.IH, g.IW, g.C, n, h0 / 2 - P / 2,
                                               w0 / 2 - P / 2, c0);
      __syncthreads();
#pragma unroll 1
      for (int it = threadIdx.x; it < (DT / 2) * (DT / 2) * D::G; it += kDwkThreads) {
        const int gi = it % D::G, pt = it / D::G;
        const int pc = pt % (DT / 2), pr = pt / (DT / 2);
        const int c = c0 + gi * 8;
        float acc[2][2][8];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[a][b][q] = 0.f;
#pragma unroll
        for (int dr = 0; dr < NW; ++dr) {
          float dv[NW][8];
#pragma unroll
          for (int dc = 0; dc < NW; ++dc)
            lds_get<T>(halo, ((pr + dr) * D::DHS + pc + dc) * D::G + gi, dv[dc]);
#pragma unroll
          for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int kh = 0; kh < K; ++kh) {
              if (((a + P - kh) & 1) != 0 || (a + P - kh) / 2 + P / 2 != dr) continue;
#pragma unroll
              for (int b = 0; b < 2; ++b) {
#pragma unroll
                for (int kw = 0; kw < K; ++kw) {
                  if (((b + P - kw) & 1) != 0) continue;
                  const int dc = (b + P - kw) / 2 + P / 2;
                  float wv[8];
                  lds_get<T>(wlv, (kh * K + kw) * D::G + gi, wv);
#pragma unroll
                  for (int q = 0; q < 8; ++q) acc[a][b][q] = fmaf(dv[dc][q], wv[q], acc[a][b][q]);
                }
              }
            }
          }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int h = h0 + 2 * pr + a, ww = w0 + 2 * pc + b;
            const long off =
                (((long)n * g.OH + min(h, g.OH - 1)) * g.OW + min(ww, g.OW - 1)) * g.C + min(c, g.C - 8);
            if constexpr (ADD) {
              float f[8];
              unpack_raw(ld_raw8(addend + off), f);
#pragma unroll
              for (int q = 0; q < 8; ++q) acc[a][b][q] += f[q];
            }
            if (h < g.OH && ww < g.OW && c < g.C) store8(dx + off, acc[a][b]);
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------- weight-grad
template <class T, int K, int S>
__global__ __launch_bounds__(kDwkThreads) void dwconvk_wgrad_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ ws_w, DwkGeom g) {
  using D = DwK<T, K, S>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* halo = reinterpret_cast<uint4*>(smem);
  uint4* dyt = reinterpret_cast<uint4*>(smem + D::HALO_BYTES);  // [TH][TW][G]
  const int c0 = blockIdx.y * D::CB;
  const int gi = threadIdx.x % D::G, t = threadIdx.x / D::G;
  const int kh = t % D::KS, rg = t / D::KS;  // slots kh >= K only help to fill

  float acc[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[k][q] = 0.f;

  for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int n, h0, w0;
    tile_pos<D::TH, D::TW>(g, tile, n, h0, w0);
    __syncthreads();
    fill_patch<T, D::HR, D::HC, D::HS, D::FOLD ? D::HRH : 0>(x, halo, g.IH, g.IW, g.C, n,
                                                             h0 * S - D::P, w0 * S - D::P, c0);
    fill_patch<T, D::TH, D::TW, D::TW, 0>(dy, dyt, g.OH, g.OW, g.C, n, h0, w0, c0);
    __syncthreads();
    if (kh < K) {
#pragma unroll 1
      for (int r = rg; r < D::TH; r += D::RG) {
        const int xb = (D::lrow(r * S + kh) * D::HS) * D::G + gi;
        const int db = (r * D::TW) * D::G + gi;
        float xw[K][8];  // the window's column col sits in slot col % K
#pragma unroll
        for (int k = 0; k < K - S; ++k) lds_get<T>(halo, xb + k * D::G, xw[k]);
#pragma unroll
        for (int wq = 0; wq < D::TW; ++wq) {
#pragma unroll
          for (int s = 0; s < S; ++s) {
            const int col = wq * S + K - S + s;
            lds_get<T>(halo, xb + col * D::G, xw[col % K]);
          }
          float dv[8];
          lds_get<T>(dyt, db + wq * D::G, dv);
#pragma unroll
          for (int kw = 0; kw < K; ++kw)
#pragma unroll
            for (int q = 0; q < 8; ++q)
              acc[kw][q] = fmaf(dv[q], xw[(wq * S + kw) % K][q], acc[kw][q]);
          // two columns in flight are enough: more of the row's LDS reads hoisted above the
          // FMAs would only cost registers
          if (wq % 2 == 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  // the block's row groups, added in index order: red[rg][g][kh][kw][q]
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  if (kh < K) {
    float* dst = red + (((rg * D::G + gi) * K + kh) * K) * 8;
#pragma unroll
    for (int kw = 0; kw < K; ++kw)
#pragma unroll
      for (int q = 0; q < 8; ++q) dst[kw * 8 + q] = acc[kw][q];
  }
  __syncthreads();
  const long prow = blockIdx.x;
  for (int o = threadIdx.x; o < D::CB * D::KK; o += kDwkThreads) {
    const int cl = o / D::KK, tap = o - cl * D::KK;
    const int gq = cl / 8, q = cl % 8;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < D::RG; ++k) s += red[((k * D::G + gq) * D::KK + tap) * 8 + q];
    if (c0 + cl < g.C) ws_w[(prow * g.C + c0 + cl) * D::KK + tap] = s;
  }
}

// tiles of th x tw over the oh x ow tensor; patches come from the ih x iw tensor
inline DwkGeom dwk_geom(int N, int C, int ih, int iw, int oh, int ow, int th, int tw) {
  DwkGeom g;
  const int nth = (oh + th - 1) / th, ntw = (ow + tw - 1) / tw;
  g.ftw = FastDiv((uint32_t)ntw);
  g.fth = FastDiv((uint32_t)nth);
  g.N = N; g.C = C; g.IH = ih; g.IW = iw; g.OH = oh; g.OW = ow;
  g.ntiles = (uint32_t)((long)N * nth * ntw);
  return g;
}

// f(T{}, K, S as integral constants) for the supported (k, s)
template <class F>
inline void dispatch_dwk(bool f32, int k, int s, F&& f) {
  dispatch_act(f32, [&](auto t) {
    dispatch_int<3, 5>(k, [&](auto kk) {
      dispatch_int<1, 2>(s, [&](auto ss) { f(t, kk, ss); });
    });
  });
}

}  // namespace

int dwk_lds_bytes(int pass, int k, int s) {
  int b = 0;
  if (!dwk_supported(k, s)) return b;
  dispatch_dwk(false, k, s, [&](auto t, auto kk, auto ss) {  // (the same for bf16 and fp32)
    using D = DwK<decltype(t), decltype(kk)::value, decltype(ss)::value>;
    b = pass == 2 ? D::WGRAD_LDS : pass == 1 && D::FOLD ? D::DGRAD2_LDS : D::FWD_LDS;
  });
  return b;
}

void dwconvk_fwd(const void* x, const void* w, const float* shift, void* y, float* ws, float* ps,
                 float* pss, int N, int H, int W, int C, int k, int s, bool f32, hipStream_t st) {
  if ((long)N * H * W * C <= 0 || !dwk_supported(k, s)) return;
  const int Ho = dwk_out(H, k, s), Wo = dwk_out(W, k, s);
  const DwkGeom g = dwk_geom(N, C, H, W, Ho, Wo, dwk_tile_h(k, s), dwk_tile_w(k, s));
  const int P = dwk_stat_rows(N, Ho, Wo, k, s);
  float* ws_q = ws == nullptr ? nullptr : ws + (long)P * C;
  dispatch_dwk(f32, k, s, [&](auto t, auto kk, auto ss) {
    using T = decltype(t);
    constexpr int K = decltype(kk)::value, S = decltype(ss)::value;
    using D = DwK<T, K, S>;
    const dim3 grid(P, (C + D::CB - 1) / D::CB);
    dispatch_bool(shift != nullptr, [&](auto stats) {
      hipLaunchKernelGGL((dwconvk_fwd_kernel<T, K, S, decltype(stats)::value>), grid,
                         dim3(kDwkThreads), D::FWD_LDS, st, (const T*)x, (const T*)w, shift, (T*)y,
                         ws, ws_q, g);
    });
  });
  if (shift != nullptr) det_sum_rows(ws, ws_q, P, C, ps, pss, false, st);
}

void dwconvk_dgrad(const void* dy, const void* w, const void* addend, void* dx, int N, int H,
                   int W, int C, int k, int s, bool f32, hipStream_t st) {
  if ((long)N * H * W * C <= 0 || !dwk_supported(k, s)) return;
  const int Ho = dwk_out(H, k, s), Wo = dwk_out(W, k, s);
  const DwkGeom g = s == 1 ? dwk_geom(N, C, H, W, H, W, dwk_tile_h(k, 1), dwk_tile_w(k, 1))
                           : dwk_geom(N, C, Ho, Wo, H, W, kDwkDgradTile, kDwkDgradTile);
  dispatch_dwk(f32, k, s, [&](auto t, auto kk, auto ss) {
    using T = decltype(t);
    constexpr int K = decltype(kk)::value, S = decltype(ss)::value;
    using D = DwK<T, K, S>;
    const dim3 grid(std::min<uint32_t>(g.ntiles, kDwkMaxBlocks), (C + D::CB - 1) / D::CB);
    dispatch_bool(addend != nullptr, [&](auto add) {
      hipLaunchKernelGGL((dwconvk_dgrad_kernel<T, K, S, decltype(add)::value>), grid,
                         dim3(kDwkThreads), S == 1 ? D::FWD_LDS : D::DGRAD2_LDS, st, (const T*)dy,
                         (const T*)w, (const T*)addend, (T*)dx, g);
    });
  });
}

void dwconvk_wgrad(const void* dy, const void* x, float* ws, float* dw, int N, int H, int W, int C,
                   int k, int s, bool f32, hipStream_t st) {
  if ((long)N * H * W * C <= 0 || !dwk_supported(k, s)) return;
  const int Ho = dwk_out(H, k, s), Wo = dwk_out(W, k, s);
  const DwkGeom g = dwk_geom(N, C, H, W, Ho, Wo, dwk_tile_h(k, s), dwk_tile_w(k, s));
  const int P = dwk_wgrad_rows(N, Ho, Wo, C, k, s, f32);
  dispatch_dwk(f32, k, s, [&](auto t, auto kk, auto ss) {
    using T = decltype(t);
    constexpr int K = decltype(kk)::value, S = decltype(ss)::value;
    using D = DwK<T, K, S>;
    const dim3 grid(P, (C + D::CB - 1) / D::CB);
    hipLaunchKernelGGL((dwconvk_wgrad_kernel<T, K, S>), grid, dim3(kDwkThreads), D::WGRAD_LDS, st,
                       (const T*)dy, (const T*)x, ws, g);
  });
  det_sum_rows(ws, nullptr, P, C * k * k, dw, nullptr, true, st);
}

}  // namespace mipipe
