// ConvNeXt block kernels: the 7x7 depthwise convolution (stride 1, pad 3, NHWC) forward,
// data-grad and weight-grad, and the block's closing layer scale + stochastic depth + residual.
//
//   dwconv7_kernel        A block owns a TH x TW output tile of one channel block (128 bytes of
//                         channels).  The (TH+6) x (TW+6) input halo is filled into LDS ONCE, every
//                         load issued unconditionally from a clamped address and zeroed by a select
//                         outside the image; each thread then produces 8 channels x a strip of SW
//                         outputs, walking the strip's SW+6 input columns once per filter row: one
//                         16-byte LDS read feeds up to SW x 8 FMAs.  The filter [C, 7, 7, 1] is read
//                         as it stands (16-byte loads of the block's contiguous channel range) and
//                         kept in LDS tap-major; the data-grad is the same loop with the taps
//                         mirrored at that staging, plus an optional fp32 addend before the rounding.
//   dwconv7_wgrad_kernel  The same halo plus the dy tile in LDS; a thread owns 8 channels x one
//                         filter row (7 taps) x a group of tile rows and slides a 7-column window of
//                         x along the row.  Accumulators live in registers across all the tiles a
//                         block takes; the block's row groups are added through LDS in index order
//                         and written as ONE partial row, and det_sum_rows adds the partial rows in
//                         a fixed order into the target: no float atomics, the same bits every run.
//   sr_fwd / sr_bwd       out = T(res + (f * gamma) * s_n) in three rounded operations, and its
//                         one-pass backward with the two column sums through partial rows.
//
// LDS layout of the halo: pixel-major, a pixel = 128 bytes (the channel block), a halo row padded
// to an ODD number of pixels.  The lanes of a ds_read_b128 group that do not share a pixel then sit
// an odd number of pixels apart, i.e. on the other 32 banks: conflict-free 16-byte reads
// (MI355X_MICROARCH.md, LDS).
#include "common.hpp"
#include "convnext.hpp"
#include "drop_hash.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

constexpr int kDw7Threads = 256;
constexpr int TH = kDw7TileH, TW = kDw7TileW;
constexpr int HR = TH + 6;   // halo rows
constexpr int HC = TW + 6;   // halo columns
constexpr int HS = HC + 1;   // halo row stride in pixels (odd)
static_assert(HS % 2 == 1, "the halo row stride must be an odd number of pixels");

template <class T>
struct Dw7 {
  static constexpr int CB = kDw7ChanBytes / (int)sizeof(T);  // channels per block: 64 / 32
  static constexpr int G = CB / 8;                           // 8-channel groups: 8 / 4
  static constexpr int V = (int)sizeof(T) / 2;               // uint4 per group: 1 / 2
  static constexpr int POS = kDw7Threads / G;                // threads per group: 32 / 64
  static constexpr int STRIPS = POS / TH;                    // strips per tile row: 4 / 8
  static constexpr int SW = TW / STRIPS;                     // outputs per strip: 4 / 2
  static constexpr int HALO_BYTES = HR * HS * kDw7ChanBytes;
  static constexpr int W_BYTES = 49 * CB * (int)sizeof(T);
  static constexpr int DY_BYTES = TH * TW * kDw7ChanBytes;
  // weight-grad: thread = (group, filter row kh of 8 slots, row group)
  static constexpr int RG = POS / 8;    // row groups: 4 / 8
  static constexpr int RPG = TH / RG;   // tile rows per group: 2 / 1
  static constexpr int RED_BYTES = (RG * G * 49 * 8 + RG * G * 8) * 4;
  static constexpr int FWD_LDS = HALO_BYTES + W_BYTES;
  static constexpr int WGRAD_LDS =
      HALO_BYTES + DY_BYTES > RED_BYTES ? HALO_BYTES + DY_BYTES : RED_BYTES;
  static_assert(POS % TH == 0 && TW % STRIPS == 0 && TH % RG == 0, "tile / thread shape");
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

struct Dw7Geom {
  FastDiv ftw, fth;  // tiles along W, along H
  int N, H, W, C;
  uint32_t ntiles;
};

// Fill ROWS x COLS pixels of the block's channel block into LDS (row stride STRIDE pixels) from
// the image of sample n with the patch's top-left at (h0, w0); outside the image (and past C): 0.
template <class T, int ROWS, int COLS, int STRIDE>
__device__ __forceinline__ void fill_patch(const T* __restrict__ src, uint4* lds, const Dw7Geom& g,
                                           int n, int h0, int w0, int c0) {
  using D = Dw7<T>;
  constexpr int kItems = ROWS * COLS * D::G;
  constexpr int kPer = (kItems + kDw7Threads - 1) / kDw7Threads;
  constexpr int kBatch = 5;
#pragma unroll
  for (int b0 = 0; b0 < kPer; b0 += kBatch) {
    Raw8<T> r[kBatch];
    bool ok[kBatch];
    int dst[kBatch];
#pragma unroll
    for (int k = 0; k < kBatch; ++k) {
      if (b0 + k < kPer) {
        const int i = (int)threadIdx.x + (b0 + k) * kDw7Threads;
        const int ic = min(i, kItems - 1);
        const int gi = ic % D::G, pix = ic / D::G;
        const int pc = pix % COLS, pr = pix / COLS;
        const int h = h0 + pr, w = w0 + pc, c = c0 + gi * 8;
        ok[k] = h >= 0 && h < g.H && w >= 0 && w < g.W && c < g.C;
        const int hc = min(max(h, 0), g.H - 1), wc = min(max(w, 0), g.W - 1), cc = min(c, g.C - 8);
        r[k] = ld_raw8(src + (((long)n * g.H + hc) * g.W + wc) * g.C + cc);
        dst[k] = i < kItems ? (pr * STRIDE + pc) * D::G + gi : -1;
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

__device__ __forceinline__ void tile_pos(const Dw7Geom& g, uint32_t tile, int& n, int& h0, int& w0) {
  const uint32_t t = g.ftw.div(tile);
  w0 = (int)(tile - t * g.ftw.d) * TW;
  const uint32_t nn = g.fth.div(t);
  h0 = (int)(t - nn * g.fth.d) * TH;
  n = (int)nn;
}

// ----------------------------------------------------------------------- forward / data-grad
template <class T, bool ADD>
__global__ __launch_bounds__(kDw7Threads) void dwconv7_kernel(
    const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias,
    const T* __restrict__ addend, T* __restrict__ y, Dw7Geom g, bool flip) {
  using D = Dw7<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* halo = reinterpret_cast<uint4*>(smem);
  T* wl = reinterpret_cast<T*>(smem + D::HALO_BYTES);  // [49][CB], tap-major
  const uint4* wlv = reinterpret_cast<const uint4*>(smem + D::HALO_BYTES);
  const int c0 = blockIdx.y * D::CB;
  const int gi = threadIdx.x % D::G, pos = threadIdx.x / D::G;
  const int row = pos % TH, strip = pos / TH;
  const int c = c0 + gi * 8;

  // the block's filter rows: channels [c0, c0 + CB) x 49 taps are contiguous in [C, 7, 7, 1]
  {
    const int nvalid = min(D::CB, g.C - c0) * 49;  // a multiple of 8
    for (int v = threadIdx.x; v < D::CB * 49 / 8; v += kDw7Threads) {
      const int e0 = v * 8;
      float f[8];
      unpack_raw(ld_raw8(w + (long)c0 * 49 + min(e0, nvalid - 8)), f);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = e0 + q;
        const int cl = e / 49, tap = e - cl * 49;
        wl[(flip ? 48 - tap : tap) * D::CB + cl] = from_f32<T>(e0 < nvalid ? f[q] : 0.f);
      }
    }
  }
  float bv[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) bv[q] = 0.f;
  if (bias != nullptr) ld_f32x8(bias + min(c, g.C - 8), bv);

  for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int n, h0, w0;
    tile_pos(g, tile, n, h0, w0);
    __syncthreads();  // the previous tile's reads are done (first pass: nothing pending)
    fill_patch<T, HR, HC, HS>(x, halo, g, n, h0 - 3, w0 - 3, c0);
    __syncthreads();  // halo and filter are in LDS

    float acc[D::SW][8];
#pragma unroll
    for (int o = 0; o < D::SW; ++o)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[o][q] = bv[q];
#pragma unroll 1
    for (int kh = 0; kh < 7; ++kh) {
      float wv[7][8];
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) lds_get<T>(wlv, (kh * 7 + kw) * D::G + gi, wv[kw]);
      const int rbase = ((row + kh) * HS + strip * D::SW) * D::G + gi;
#pragma unroll
      for (int j = 0; j < D::SW + 6; ++j) {
        float xv[8];
        lds_get<T>(halo, rbase + j * D::G, xv);
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) {
          const int o = j - kw;
          if (o >= 0 && o < D::SW) {
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[o][q] = fmaf(xv[q], wv[kw][q], acc[o][q]);
          }
        }
      }
    }
    const int h = h0 + row, wbase = w0 + strip * D::SW;
    const long rowoff = ((long)n * g.H + min(h, g.H - 1)) * g.W;
    if constexpr (ADD) {
      Raw8<T> a[D::SW];
#pragma unroll
      for (int o = 0; o < D::SW; ++o)
        a[o] = ld_raw8(addend + (rowoff + min(wbase + o, g.W - 1)) * g.C + min(c, g.C - 8));
#pragma unroll
      for (int o = 0; o < D::SW; ++o) {
        float f[8];
        unpack_raw(a[o], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[o][q] += f[q];
      }
    }
    if (h < g.H && c < g.C) {
#pragma unroll
      for (int o = 0; o < D::SW; ++o)
        if (wbase + o < g.W) store8(y + (rowoff + wbase + o) * g.C + c, acc[o]);
    }
  }
}

// ------------------------------------------------------------------------------- weight-grad
template <class T>
__global__ __launch_bounds__(kDw7Threads) void dwconv7_wgrad_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ ws_w,
    float* __restrict__ ws_b, Dw7Geom g) {
  using D = Dw7<T>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* halo = reinterpret_cast<uint4*>(smem);
  uint4* dyt = reinterpret_cast<uint4*>(smem + D::HALO_BYTES);  // [TH][TW][G]
  const int c0 = blockIdx.y * D::CB;
  const int gi = threadIdx.x % D::G, t = threadIdx.x / D::G;
  const int kh = t % 8, rg = t / 8;  // slot kh == 7 only helps to fill

  float acc[7][8], bacc[8];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[k][q] = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) bacc[q] = 0.f;

  for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int n, h0, w0;
    tile_pos(g, tile, n, h0, w0);
    __syncthreads();
    fill_patch<T, HR, HC, HS>(x, halo, g, n, h0 - 3, w0 - 3, c0);
    fill_patch<T, TH, TW, TW>(dy, dyt, g, n, h0, w0, c0);
    __syncthreads();
    if (kh < 7) {
#pragma unroll 1
      for (int rr = 0; rr < D::RPG; ++rr) {
        const int r = rg * D::RPG + rr;
        const int xb = ((r + kh) * HS) * D::G + gi;
        const int db = (r * TW) * D::G + gi;
        float xw[7][8];
#pragma unroll
        for (int k = 0; k < 6; ++k) lds_get<T>(halo, xb + k * D::G, xw[k]);
#pragma unroll
        for (int wq = 0; wq < TW; ++wq) {
          lds_get<T>(halo, xb + (wq + 6) * D::G, xw[(wq + 6) % 7]);
          float dv[8];
          lds_get<T>(dyt, db + wq * D::G, dv);
#pragma unroll
          for (int kw = 0; kw < 7; ++kw)
#pragma unroll
            for (int q = 0; q < 8; ++q)
              acc[kw][q] = fmaf(dv[q], xw[(wq + kw) % 7][q], acc[kw][q]);
          if (kh == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) bacc[q] += dv[q];
          }
          // keep the scheduler from hoisting the whole row's LDS reads (and their unpacked
          // values) above the FMAs: two columns in flight are enough, more would spill
          if (wq % 2 == 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  }
  // the block's row groups, added in index order: red[rg][g][kh][kw][q], redb[rg][g][q]
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);
  float* redb = red + D::RG * D::G * 49 * 8;
  if (kh < 7) {
    float* dst = red + (((rg * D::G + gi) * 7 + kh) * 7) * 8;
#pragma unroll
    for (int kw = 0; kw < 7; ++kw)
#pragma unroll
      for (int q = 0; q < 8; ++q) dst[kw * 8 + q] = acc[kw][q];
    if (kh == 0) {
#pragma unroll
      for (int q = 0; q < 8; ++q) redb[(rg * D::G + gi) * 8 + q] = bacc[q];
    }
  }
  __syncthreads();
  const long prow = blockIdx.x;
  for (int o = threadIdx.x; o < D::CB * 49; o += kDw7Threads) {
    const int cl = o / 49, tap = o - cl * 49;
    const int gq = cl / 8, q = cl % 8;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < D::RG; ++k) s += red[((k * D::G + gq) * 49 + tap) * 8 + q];
    if (c0 + cl < g.C) ws_w[(prow * g.C + c0 + cl) * 49 + tap] = s;
  }
  if (threadIdx.x < D::CB) {
    const int cl = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < D::RG; ++k) s += redb[(k * D::G + cl / 8) * 8 + cl % 8];
    if (c0 + cl < g.C) ws_b[prow * g.C + c0 + cl] = s;
  }
}

inline Dw7Geom dw7_geom(int N, int H, int W, int C) {
  Dw7Geom g;
  g.ftw = FastDiv((uint32_t)((W + TW - 1) / TW));
  g.fth = FastDiv((uint32_t)((H + TH - 1) / TH));
  g.N = N; g.H = H; g.W = W; g.C = C;
  g.ntiles = (uint32_t)dw7_tiles(N, H, W);
  return g;
}

// -------------------------------------------------------------------------- scale_residual
constexpr int kSrThreads = kSrFwdThreads;  // both directions run 256-thread blocks
constexpr int kSrItems = kSrFwdItems;

// (a * b) * s, and r + that: each operation rounded (hipcc would contract the add into an FMA)
__device__ __forceinline__ float sr_scaled(float a, float b, float s) {
#pragma clang fp contract(off)
  const float t = a * b;
  return t * s;
}
__device__ __forceinline__ float sr_add(float r, float v) {
#pragma clang fp contract(off)
  return r + v;
}

template <class T>
__global__ __launch_bounds__(kSrThreads) void sr_fwd_kernel(
    const T* __restrict__ f, const T* __restrict__ res, const float* __restrict__ gamma,
    T* __restrict__ out, uint32_t items, FastDiv fC8, FastDiv fHW, PathDrop d) {
  constexpr uint32_t kTile = kSrThreads * kSrItems;
  const uint32_t base = drop_base(d.seed, d.seed_dev);
  for (uint32_t t0 = blockIdx.x * kTile; t0 < items; t0 += gridDim.x * kTile) {
    Raw8<T> rf[kSrItems], rr[kSrItems];
    float gm[kSrItems][8], s[kSrItems];
#pragma unroll
    for (int k = 0; k < kSrItems; ++k) {
      const uint32_t o = min(t0 + threadIdx.x + k * kSrThreads, items - 1);
      const uint32_t r = fC8.div(o);
      const uint32_t cg = o - r * fC8.d;
      rf[k] = ld_raw8(f + (long)o * 8);
      rr[k] = ld_raw8(res + (long)o * 8);
      ld_f32x8(gamma + cg * 8, gm[k]);
      s[k] = drop_keep(base, (long)fHW.div(r), d.thr) ? d.scale : 0.f;
    }
#pragma unroll
    for (int k = 0; k < kSrItems; ++k) {
      const uint32_t o = t0 + threadIdx.x + k * kSrThreads;
      float a[8], b[8];
      unpack_raw(rf[k], a);
      unpack_raw(rr[k], b);
#pragma unroll
      for (int q = 0; q < 8; ++q) b[q] = sr_add(b[q], sr_scaled(a[q], gm[k][q], s[k]));
      if (o < items) store8(out + (long)o * 8, b);
    }
  }
}

// Block (x, y): column chunk y of 64 channels; thread = 8 channels x row lane (32 lanes), 4 rows
// per lane and pass with their loads in flight together.  One partial row per block x.
template <class T, bool BIAS>
__global__ __launch_bounds__(kSrThreads) void sr_bwd_kernel(
    const T* __restrict__ dout, const T* __restrict__ f, const float* __restrict__ gamma,
    T* __restrict__ df, float* __restrict__ ws_g, float* __restrict__ ws_b, long R, int C,
    FastDiv fHW, PathDrop d) {
  __shared__ float red[2][32][65];
  const int gi = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int c = blockIdx.y * 64 + gi * 8;
  const bool cok = c < C;
  const int cc = min(c, C - 8);
  const uint32_t base = drop_base(d.seed, d.seed_dev);
  float gm[8], ag[8], ab[8];
  ld_f32x8(gamma + cc, gm);
#pragma unroll
  for (int q = 0; q < 8; ++q) ag[q] = ab[q] = 0.f;
  for (long r0 = (long)blockIdx.x * kSrBlockRows; r0 < R; r0 += (long)gridDim.x * kSrBlockRows) {
    Raw8<T> rd[4], rf[4];
    float s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long r = min(r0 + rl + 32 * k, R - 1);
      rd[k] = ld_raw8(dout + r * C + cc);
      rf[k] = ld_raw8(f + r * C + cc);
      s[k] = drop_keep(base, (long)fHW.div((uint32_t)r), d.thr) ? d.scale : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long r = r0 + rl + 32 * k;
      const bool ok = r < R;
      float a[8], b[8], o[8];
      unpack_raw(rd[k], a);
      unpack_raw(rf[k], b);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        o[q] = sr_scaled(a[q], gm[q], s[k]);
        const float tg = sr_scaled(a[q], b[q], s[k]);
        ag[q] += ok ? tg : 0.f;
        if (BIAS) ab[q] += ok ? as_stored<T>(o[q]) : 0.f;
      }
      if (ok && cok) store8(df + r * C + c, o);
    }
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    red[0][rl][gi * 8 + q] = ag[q];
    if (BIAS) red[1][rl][gi * 8 + q] = ab[q];
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    const int col = blockIdx.y * 64 + threadIdx.x;
    float sg = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      sg += red[0][k][threadIdx.x];
      if (BIAS) sb += red[1][k][threadIdx.x];
    }
    if (col < C) {
      ws_g[(long)blockIdx.x * C + col] = sg;
      if (BIAS) ws_b[(long)blockIdx.x * C + col] = sb;
    }
  }
}

}  // namespace

void dwconv7_fwd(const void* x, const void* w, const float* bias, const void* addend, void* y,
                 int N, int H, int W, int C, bool flip, bool f32, hipStream_t st) {
  if ((long)N * H * W * C <= 0) return;
  const Dw7Geom g = dw7_geom(N, H, W, C);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    using D = Dw7<T>;
    const dim3 grid(std::min<uint32_t>(g.ntiles, kDw7MaxBlocks), (C + D::CB - 1) / D::CB);
    dispatch_bool(addend != nullptr, [&](auto add) {
      hipLaunchKernelGGL((dwconv7_kernel<T, decltype(add)::value>), grid, dim3(kDw7Threads),
                         D::FWD_LDS, st, (const T*)x, (const T*)w, bias, (const T*)addend, (T*)y,
                         g, flip);
    });
  });
}

void dwconv7_wgrad(const void* dy, const void* x, float* ws_w, float* ws_b, float* dw, float* db,
                   int N, int H, int W, int C, bool f32, hipStream_t st) {
  if ((long)N * H * W * C <= 0) return;
  const Dw7Geom g = dw7_geom(N, H, W, C);
  const int P = dw7_wgrad_rows(N, H, W, C, f32);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    using D = Dw7<T>;
    const dim3 grid(P, (C + D::CB - 1) / D::CB);
    hipLaunchKernelGGL(dwconv7_wgrad_kernel<T>, grid, dim3(kDw7Threads), D::WGRAD_LDS, st,
                       (const T*)dy, (const T*)x, ws_w, ws_b, g);
  });
  det_sum_rows(ws_w, nullptr, P, C * 49, dw, nullptr, true, st);
  det_sum_rows(ws_b, nullptr, P, C, db, nullptr, true, st);
}

void scale_residual_fwd(const void* f, const void* res, const float* gamma, void* out, long R,
                        int C, int HW, PathDrop d, bool f32, hipStream_t st) {
  if (R <= 0 || C <= 0) return;
  const uint32_t items = (uint32_t)(R * (C / 8));
  const uint32_t tile = kSrThreads * kSrItems;
  const int grid = (int)std::max<uint32_t>(1, std::min<uint32_t>((items + tile - 1) / tile,
                                                                 kSrFwdMaxBlocks));
  const FastDiv fC8((uint32_t)C / 8), fHW((uint32_t)HW);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(sr_fwd_kernel<T>, dim3(grid), dim3(kSrThreads), 0, st, (const T*)f,
                       (const T*)res, gamma, (T*)out, items, fC8, fHW, d);
  });
}

void scale_residual_bwd(const void* dout, const void* f, const float* gamma, void* df, float* ws_g,
                        float* ws_b, float* dgamma, float* dbias, long R, int C, int HW,
                        PathDrop d, bool f32, hipStream_t st) {
  if (R <= 0 || C <= 0) return;
  const int P = sr_bwd_rows(R, C);
  const dim3 grid(P, (C + 63) / 64);
  const FastDiv fHW((uint32_t)HW);
  const bool with_bias = dbias != nullptr;
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    dispatch_bool(with_bias, [&](auto b) {
      hipLaunchKernelGGL((sr_bwd_kernel<T, decltype(b)::value>), grid, dim3(kSrThreads), 0, st,
                         (const T*)dout, (const T*)f, gamma, (T*)df, ws_g, ws_b, R, C, fHW, d);
    });
  });
  det_sum_rows(ws_g, with_bias ? ws_b : nullptr, P, C, dgamma, with_bias ? dbias : nullptr, true,
               st);
}

}  // namespace mipipe
