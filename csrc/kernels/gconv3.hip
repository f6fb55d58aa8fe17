// Grouped 3 x 3 convolution on MFMA for small group widths (RegNet's f.b): Cin = Cout = C,
// G = C / groups with G % 8 == 0 and 8 <= G <= 64, pad 1, stride S in {1, 2}, no bias, NHWC, bf16.
// The weight is gconv's operand [C, 3, 3, G], read as it stands.  Channel blocks of whole groups
// (64 / G groups, at most 64 channels) go in grid.y, spatial tiles in grid.x (grid-strided).
//
//   gconv3_fwd_kernel    A block owns a TH x TW OUTPUT tile (8 x 16 at S = 1, 8 x 8 at S = 2) of one
//                        channel block.  The input halo is filled into LDS once, pixel-major (a
//                        pixel = 144 bytes: 64 channels + 16 bytes, so the 16-byte reads of
//                        neighbouring pixels start 36 banks apart), loads clamped and zeroed by a
//                        select; the block's weight rows are staged once per block.  Each group is
//                        an implicit GEMM on mfma_f32_16x16x32_bf16 in the swapped orientation:
//                        weight rows are the row operand, 16 pixels the column operand, K = 9 G
//                        flattened tap-major, so a lane's 8-element k-run is ONE 16-byte LDS read
//                        of one halo pixel at one tap and its 4 accumulators are 4 consecutive
//                        channels of one pixel (8-byte stores).  Past K both fragments are selected
//                        to zero (0 * NaN is not 0).  Output rows are padded to 16 (G = 24, 40, 56).
//                        With STATS a lane keeps sum (v - shift) and its square of the values it
//                        STORED; the 16 pixel lanes are added by DPP, the 4 waves through LDS in
//                        index order into one partial row per block: det_sum_rows adds the rows.
//   gconv3_dgrad_kernel  S = 1: the forward loop over dy; the weight is transposed within its
//                        group and its taps mirrored while it is staged.
//   gconv3_dgrad2_kernel S = 2: a block owns a 16 x 16 tile of dx and a 9 x 9 halo of dy.  The four
//                        parity classes (a, b) of dx are four GEMMs with (1 + a)(1 + b) taps
//                        (K = G, 2G, 2G, 4G), 64 pixels each, one 16-pixel block per wave.
//   gconv3_wgrad_kernel  dW[co][ci][tap] = sum over pixels dy[p][co] x[p + tap][ci]: the x halo
//                        and the dy tile sit in LDS, the pixel axis is the MFMA's K, and both
//                        fragments come from transposed LDS reads (ds_read_b64_tr_b16: a lane
//                        gives the address of pixel k0 + (lane & 15) / 4 at 4 channels and receives
//                        4 pixels of channel lane & 15), whose per-lane row addresses make the tap
//                        shift free.  A wave owns (group, 16-ci block) units x 9 taps x all co
//                        blocks; the accumulators stay in registers over all the tiles the block
//                        walks and are written once into the block's partial slab, laid out as the
//                        target ([C, G, 3, 3], or its channels-last order [C, 3, 3, G], which is
//                        how the parameter and its flat gradient are stored); det_sum_rows adds
//                        the slabs into it.
// No float atomics anywhere: every launch gives the same bits.
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

constexpr int kGc3Threads = 256;
constexpr int kPixB = 144;  // LDS bytes of a pixel: 64 channels + 16 bytes of padding

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

template <int G>
struct GCfg {
  static_assert(G % 8 == 0 && G >= 8 && G <= 64, "group width");
  static constexpr int NG = gc3_groups_per_block(G);  // groups of a channel block
  static constexpr int CB = NG * G;                   // its channels (<= 64)
  static constexpr int CH8 = CB / 8;                  // 16-byte chunks of a pixel
  static constexpr int GP = (G + 15) / 16 * 16;       // output rows of a group, padded
  static constexpr int CBS = GP / 16;                 // 16-row blocks of a group
  static constexpr int WROW = 9 * G + 8;              // elements of a weight row in LDS
  static constexpr int W_BYTES = NG * GP * WROW * 2;
};

template <int S>
struct GTile {
  static constexpr int TH = 8, TW = S == 1 ? 16 : 8;  // gc3_tile_h / gc3_tile_w
  static constexpr int HR = (TH - 1) * S + 3, HC = (TW - 1) * S + 3;
  static constexpr int HALO_BYTES = HR * HC * kPixB;
  static constexpr int NPIX = TH * TW;
  static constexpr int NPB = NPIX / 16 / 4;  // 16-pixel blocks per wave
  static constexpr int DY_BYTES = NPIX * kPixB;
};
constexpr int kDT = kGc3DgradTile;      // stride-2 data-grad: tile of dx
constexpr int kDHR = kDT / 2 + 1;       // and its halo of dy (rows = columns)
constexpr int kDHaloBytes = kDHR * kDHR * kPixB;

struct Gc3Geom {
  FastDiv ftw, fth;  // tiles along W, along H
  int N, C;
  int IH, IW;  // the tensor the LDS halo is filled from
  int OH, OW;  // the tensor the tiles cover
  uint32_t ntiles;
};

template <int TH, int TW>
__device__ __forceinline__ void tile_pos(const Gc3Geom& g, uint32_t tile, int& n, int& h0, int& w0) {
  const uint32_t t = g.ftw.div(tile);
  w0 = (int)(tile - t * g.ftw.d) * TW;
  const uint32_t nn = g.fth.div(t);
  h0 = (int)(t - nn * g.fth.d) * TH;
  n = (int)nn;
}

// ROWS x COLS pixels x CH8 chunks of the block's channels into LDS from the ih x iw image of
// sample n, the patch's top-left at (h0, w0); outside the image or past C: 0 (by a select: the
// load itself goes to a clamped address).
template <int ROWS, int COLS, int CH8>
__device__ __forceinline__ void fill_patch(const __bf16* __restrict__ src, char* lds, int ih, int iw,
                                           int C, int n, int h0, int w0, int c0) {
  constexpr int kItems = ROWS * COLS * CH8;
#pragma unroll 4
  for (int it = threadIdx.x; it < kItems; it += kGc3Threads) {
    const int gi = it % CH8, pix = it / CH8;
    const int pc = pix % COLS, pr = pix / COLS;
    const int h = h0 + pr, w = w0 + pc, c = c0 + gi * 8;
    const bool ok = h >= 0 && h < ih && w >= 0 && w < iw && c < C;
    const int hc = min(max(h, 0), ih - 1), wc = min(max(w, 0), iw - 1), cc = min(c, C - 8);
    const uint4 v = *reinterpret_cast<const uint4*>(src + (((long)n * ih + hc) * iw + wc) * C + cc);
    *reinterpret_cast<uint4*>(lds + pix * kPixB + gi * 16) = ok ? v : make_uint4(0u, 0u, 0u, 0u);
  }
}

// The block's weight rows into LDS: wl[group][row][tap * G + col], rows past G (and the rows of
// groups past C) zero.  Forward: row = co, col = ci, a straight copy of [C, 3, 3, G].  TRANS
// (data-grad): row = ci, col = co; FLIP: tap -> 8 - tap.
template <int G, bool TRANS, bool FLIP>
__device__ __forceinline__ void stage_weights(const __bf16* __restrict__ w, char* wl, int C, int c0) {
  using Cf = GCfg<G>;
  constexpr int kRowChunks = 9 * G / 8;
  uint16_t* wl16 = reinterpret_cast<uint16_t*>(wl);
  if constexpr (TRANS || Cf::GP != G) {  // rows the copy below does not write
    for (int v = threadIdx.x; v < Cf::NG * Cf::GP * kRowChunks; v += kGc3Threads) {
      const int row = v / kRowChunks, ch = v - row * kRowChunks;
      const int gr = row / Cf::GP, m = row - gr * Cf::GP;
      if (m >= G || c0 + gr * G >= C)
        *reinterpret_cast<uint4*>(wl + (row * Cf::WROW + ch * 8) * 2) = make_uint4(0u, 0u, 0u, 0u);
    }
  }
  for (int v = threadIdx.x; v < Cf::NG * G * kRowChunks; v += kGc3Threads) {
    const int row = v / kRowChunks, ch = v - row * kRowChunks;  // row: a channel of the block
    const int gr = row / G, m = row - gr * G;
    const bool ok = c0 + gr * G < C;
    const int rc = min(c0 + row, C - 1);
    const uint4 u = *reinterpret_cast<const uint4*>(w + (long)rc * 9 * G + ch * 8);
    if constexpr (!TRANS) {
      *reinterpret_cast<uint4*>(wl + ((gr * Cf::GP + m) * Cf::WROW + ch * 8) * 2) =
          ok ? u : make_uint4(0u, 0u, 0u, 0u);
    } else if (ok) {
      const int tap = (ch * 8) / G, ci0 = ch * 8 - tap * G;
      const int tp = FLIP ? 8 - tap : tap;
      const uint32_t e[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int q = 0; q < 8; ++q)
        wl16[(gr * Cf::GP + ci0 + q) * Cf::WROW + tp * G + m] =
            (uint16_t)(q & 1 ? e[q >> 1] >> 16 : e[q >> 1] & 0xffffu);
    }
  }
}

// Flattened tap t -> halo offset in pixels and the weight's tap
template <int HS>
struct DecConv {  // the 9 taps of a 3 x 3 window whose corner is the lane's base pixel
  static constexpr int NT = 9;
  __device__ static __forceinline__ void decode(int t, int& hoff, int& wtap) {
    const int kh = t / 3, kw = t - 3 * kh;
    hoff = kh * HS + kw;
    wtap = t;
  }
};
// Parity class (A, B) of the stride-2 data-grad: dx[2 pr + A][2 pc + B] takes kh = 1 from dy row
// pr (A = 0) or kh = 0, 2 from dy rows pr + 1, pr (A = 1); likewise kw by B
template <int HS, int A, int B>
struct DecCls {
  static constexpr int NT = (1 + A) * (1 + B);
  __device__ static __forceinline__ void decode(int t, int& hoff, int& wtap) {
    const int jh = B ? t >> 1 : t, jw = B ? t & 1 : 0;
    const int kh = A ? 2 * jh : 1, dr = A ? 1 - jh : 0;
    const int kw = B ? 2 * jw : 1, dc = B ? 1 - jw : 0;
    hoff = dr * HS + dc;
    wtap = kh * 3 + kw;
  }
};

// acc[p][cb] += W[16 cb .. +16][K] * X[K][16 pixels of block p] for one group: K = NT * G, k-run
// of a lane = 8 channels of one tap.  xg: the halo at the group's first channel, wg: the group's
// weight rows, pbase[p]: byte offset of the lane's pixel of block p.
template <int G, int NPB, class Dec>
__device__ __forceinline__ void taps_gemm(const char* xg, const char* wg, const int (&pbase)[NPB],
                                          f32x4 (&acc)[NPB][GCfg<G>::CBS]) {
  using Cf = GCfg<G>;
  constexpr int KB = (Dec::NT * G + 31) / 32;
  const int lane = threadIdx.x & 63, lg = lane >> 4, li = lane & 15;
  const bf16x8 zero = __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
#pragma unroll 2
  for (int kb = 0; kb < KB; ++kb) {
    const int k = kb * 32 + 8 * lg;
    const int t = k / G, ci = k - t * G;
    const bool ok = t < Dec::NT;
    int hoff, wtap;
    Dec::decode(ok ? t : 0, hoff, wtap);
    bf16x8 b[NPB];
#pragma unroll
    for (int p = 0; p < NPB; ++p) {
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(xg + pbase[p] + hoff * kPixB + ci * 2);
      b[p] = ok ? v : zero;
    }
#pragma unroll
    for (int cb = 0; cb < Cf::CBS; ++cb) {
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(wg + ((cb * 16 + li) * Cf::WROW + wtap * G + ci) * 2);
      const bf16x8 a = ok ? v : zero;
#pragma unroll
      for (int p = 0; p < NPB; ++p)
        acc[p][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[p], acc[p][cb], 0, 0, 0);
    }
  }
}

// 4 consecutive channels of one pixel: (+ addend) -> one rounding -> 8-byte store
template <bool ADD>
__device__ __forceinline__ void store4(__bf16* __restrict__ out, const __bf16* __restrict__ addend,
                                       long off, bool ok, const f32x4& a, float* f) {
  f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3];
  if constexpr (ADD) {
    float ad[4];
    unpack4(*reinterpret_cast<const uint2*>(addend + off), ad);
#pragma unroll
    for (int r = 0; r < 4; ++r) f[r] += ad[r];
  }
  if (ok) *reinterpret_cast<uint2*>(out + off) = pack4(f);
}

// ------------------------------------------------ forward, and the stride-1 data-grad (TRANS)
template <int G, int S, bool TRANS, bool ADD, bool STATS>
__device__ __forceinline__ void conv_tiles(const __bf16* __restrict__ x, const __bf16* __restrict__ w,
                                           const float* __restrict__ shift,
                                           const __bf16* __restrict__ addend, __bf16* __restrict__ y,
                                           float* __restrict__ ws_s, float* __restrict__ ws_q,
                                           const Gc3Geom& g, char* smem) {
  using Cf = GCfg<G>;
  using T = GTile<S>;
  char* halo = smem;
  char* wl = smem + T::HALO_BYTES;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, lg = lane >> 4, li = lane & 15;
  const int c0 = blockIdx.y * Cf::CB;
  stage_weights<G, TRANS, TRANS>(w, wl, g.C, c0);

  int prow[T::NPB], pcol[T::NPB], pbase[T::NPB];
#pragma unroll
  for (int p = 0; p < T::NPB; ++p) {
    const int q = (wave * T::NPB + p) * 16 + li;
    prow[p] = q / T::TW;
    pcol[p] = q % T::TW;
    pbase[p] = (prow[p] * S * T::HC + pcol[p] * S) * kPixB;
  }
  float ssum[Cf::NG][Cf::CBS][4], ssq[Cf::NG][Cf::CBS][4], sh[Cf::NG][Cf::CBS][4];
#pragma unroll
  for (int gr = 0; gr < Cf::NG; ++gr)
#pragma unroll
    for (int cb = 0; cb < Cf::CBS; ++cb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ssum[gr][cb][r] = ssq[gr][cb][r] = sh[gr][cb][r] = 0.f;
      if constexpr (STATS) {
        const float4 v = *reinterpret_cast<const float4*>(
            shift + min(c0 + gr * G + cb * 16 + 4 * lg, g.C - 4));
        sh[gr][cb][0] = v.x; sh[gr][cb][1] = v.y; sh[gr][cb][2] = v.z; sh[gr][cb][3] = v.w;
      }
    }

  for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int n, h0, w0;
    tile_pos<T::TH, T::TW>(g, tile, n, h0, w0);
    __syncthreads();  // the previous tile's reads are done
    fill_patch<T::HR, T::HC, Cf::CH8>(x, halo, g.IH, g.IW, g.C, n, h0 * S - 1, w0 * S - 1, c0);
    __syncthreads();  // halo and weights are in LDS
#pragma unroll
    for (int gr = 0; gr < Cf::NG; ++gr) {
      if (c0 + gr * G >= g.C) break;  // (block-uniform)
      f32x4 acc[T::NPB][Cf::CBS];
#pragma unroll
      for (int p = 0; p < T::NPB; ++p)
#pragma unroll
        for (int cb = 0; cb < Cf::CBS; ++cb) acc[p][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
      taps_gemm<G, T::NPB, DecConv<T::HC>>(halo + gr * G * 2, wl + gr * Cf::GP * Cf::WROW * 2, pbase,
                                           acc);
#pragma unroll
      for (int p = 0; p < T::NPB; ++p) {
        const int h = h0 + prow[p], ww = w0 + pcol[p];
        const long pix = ((long)n * g.OH + min(h, g.OH - 1)) * g.OW + min(ww, g.OW - 1);
#pragma unroll
        for (int cb = 0; cb < Cf::CBS; ++cb) {
          const int cl = cb * 16 + 4 * lg;
          const bool ok = cl < G && h < g.OH && ww < g.OW;
          float f[4];
          store4<ADD>(y, addend, pix * g.C + min(c0 + gr * G + cl, g.C - 4), ok, acc[p][cb], f);
          if constexpr (STATS) {
            if (ok) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float v = as_stored<__bf16>(f[r]) - sh[gr][cb][r];
                ssum[gr][cb][r] += v;
                ssq[gr][cb][r] = fmaf(v, v, ssq[gr][cb][r]);
              }
            }
          }
        }
      }
    }
  }
  if constexpr (STATS) {
    // the 16 pixel lanes by DPP, then the 4 waves in index order: red[2][4][64]
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int gr = 0; gr < Cf::NG; ++gr)
#pragma unroll
      for (int cb = 0; cb < Cf::CBS; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = row16_sum(ssum[gr][cb][r]), q = row16_sum(ssq[gr][cb][r]);
          const int cl = cb * 16 + 4 * lg + r;
          if (li == 0 && cl < G) {
            red[wave * 64 + gr * G + cl] = s;
            red[(4 + wave) * 64 + gr * G + cl] = q;
          }
        }
    __syncthreads();
    if (threadIdx.x < 2 * Cf::CB) {
      const int cl = threadIdx.x % Cf::CB, a = threadIdx.x / Cf::CB;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += red[(a * 4 + k) * 64 + cl];
      if (c0 + cl < g.C) (a == 0 ? ws_s : ws_q)[(long)blockIdx.x * g.C + c0 + cl] = s;
    }
  }
}

template <int G, int S>
constexpr int conv_lds() { return GTile<S>::HALO_BYTES + GCfg<G>::W_BYTES; }

template <int G, int S, bool STATS>
__global__ __launch_bounds__(kGc3Threads) void gconv3_fwd_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ w, const float* __restrict__ shift,
    __bf16* __restrict__ y, float* __restrict__ ws_s, float* __restrict__ ws_q, Gc3Geom g) {
  __shared__ __attribute__((aligned(16))) char smem[conv_lds<G, S>()];
  conv_tiles<G, S, false, false, STATS>(x, w, shift, nullptr, y, ws_s, ws_q, g, smem);
}

template <int G, bool ADD>
__global__ __launch_bounds__(kGc3Threads) void gconv3_dgrad_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ w, const __bf16* __restrict__ addend,
    __bf16* __restrict__ dx, Gc3Geom g) {
  __shared__ __attribute__((aligned(16))) char smem[conv_lds<G, 1>()];
  conv_tiles<G, 1, true, ADD, false>(dy, w, nullptr, addend, dx, nullptr, nullptr, g, smem);
}

// ------------------------------------------------------------------- stride-2 data-grad
template <int G, bool ADD, int A, int B>
__device__ __forceinline__ void dgrad2_class(const char* xg, const char* wg, int pbase, int c,
                                             const __bf16* __restrict__ addend,
                                             __bf16* __restrict__ dx, const Gc3Geom& g, int n, int h,
                                             int w, int lg) {
  using Cf = GCfg<G>;
  f32x4 acc[1][Cf::CBS];
#pragma unroll
  for (int cb = 0; cb < Cf::CBS; ++cb) acc[0][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int pb[1] = {pbase};
  taps_gemm<G, 1, DecCls<kDHR, A, B>>(xg, wg, pb, acc);
  h += A;
  w += B;
  const long pix = ((long)n * g.OH + min(h, g.OH - 1)) * g.OW + min(w, g.OW - 1);
#pragma unroll
  for (int cb = 0; cb < Cf::CBS; ++cb) {
    const int cl = cb * 16 + 4 * lg;
    float f[4];
    store4<ADD>(dx, addend, pix * g.C + min(c + cl, g.C - 4), cl < G && h < g.OH && w < g.OW,
                acc[0][cb], f);
  }
}

template <int G, bool ADD>
__global__ __launch_bounds__(kGc3Threads) void gconv3_dgrad2_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ w, const __bf16* __restrict__ addend,
    __bf16* __restrict__ dx, Gc3Geom g) {
  using Cf = GCfg<G>;
  __shared__ __attribute__((aligned(16))) char smem[kDHaloBytes + Cf::W_BYTES];
  char* halo = smem;
  char* wl = smem + kDHaloBytes;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, lg = lane >> 4, li = lane & 15;
  const int c0 = blockIdx.y * Cf::CB;
  stage_weights<G, true, false>(w, wl, g.C, c0);
  // the wave's 16 patches (one pixel of every class each): rows 2 wave, 2 wave + 1 of the 8 x 8
  const int pr = 2 * wave + (li >> 3), pc = li & 7;
  const int pbase = (pr * kDHR + pc) * kPixB;

  for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int n, h0, w0;
    tile_pos<kDT, kDT>(g, tile, n, h0, w0);
    __syncthreads();
    fill_patch<kDHR, kDHR, Cf::CH8>(dy, halo, g.IH, g.IW, g.C, n, h0 / 2, w0 / 2, c0);
    __syncthreads();
    const int h = h0 + 2 * pr, ww = w0 + 2 * pc;
#pragma unroll
    for (int gr = 0; gr < Cf::NG; ++gr) {
      if (c0 + gr * G >= g.C) break;
      const char* xg = halo + gr * G * 2;
      const char* wg = wl + gr * Cf::GP * Cf::WROW * 2;
      const int c = c0 + gr * G;
      dgrad2_class<G, ADD, 0, 0>(xg, wg, pbase, c, addend, dx, g, n, h, ww, lg);
      dgrad2_class<G, ADD, 0, 1>(xg, wg, pbase, c, addend, dx, g, n, h, ww, lg);
      dgrad2_class<G, ADD, 1, 0>(xg, wg, pbase, c, addend, dx, g, n, h, ww, lg);
      dgrad2_class<G, ADD, 1, 1>(xg, wg, pbase, c, addend, dx, g, n, h, ww, lg);
    }
  }
}

// ------------------------------------------------------------------------------- weight-grad
// 8 k-slots (pixels) of 16 channels as an MFMA fragment: the lane's two row addresses
__device__ __forceinline__ bf16x8 tr_frag(const char* lo, const char* hi) {
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi);
  const s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}

template <int G, int S>
__global__ __launch_bounds__(kGc3Threads) void gconv3_wgrad_kernel(
    const __bf16* __restrict__ dy, const __bf16* __restrict__ x, float* __restrict__ ws, Gc3Geom g,
    int chl) {
  using Cf = GCfg<G>;
  using T = GTile<S>;
  constexpr int U = Cf::NG * Cf::CBS;  // (group, ci block) units of the block
  constexpr int UPW = (U + 3) / 4;     // per wave
  constexpr int NKS = T::NPIX / 32;    // k-steps of a tile
  __shared__ __attribute__((aligned(16))) char smem[T::HALO_BYTES + T::DY_BYTES];
  char* halo = smem;
  char* dyt = smem + T::HALO_BYTES;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, lg = lane >> 4, li = lane & 15;
  const int c0 = blockIdx.y * Cf::CB;

  f32x4 acc[UPW][9][Cf::CBS];
#pragma unroll
  for (int j = 0; j < UPW; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int cb = 0; cb < Cf::CBS; ++cb) acc[j][t][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (uint32_t tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int n, h0, w0;
    tile_pos<T::TH, T::TW>(g, tile, n, h0, w0);
    __syncthreads();
    fill_patch<T::HR, T::HC, Cf::CH8>(x, halo, g.IH, g.IW, g.C, n, h0 * S - 1, w0 * S - 1, c0);
    fill_patch<T::TH, T::TW, Cf::CH8>(dy, dyt, g.OH, g.OW, g.C, n, h0, w0, c0);
    __syncthreads();
#pragma unroll 1
    for (int ks = 0; ks < NKS; ++ks) {
      // the pixels whose addresses this lane gives: slots 8 lg + (li >> 2) and 4 further on
      const int s_lo = ks * 32 + 8 * lg + (li >> 2), s_hi = s_lo + 4;
      const int choff = 4 * (li & 3) * 2;
      const char* d_lo = dyt + s_lo * kPixB + choff;
      const char* d_hi = dyt + s_hi * kPixB + choff;
      const char* x_lo = halo + ((s_lo / T::TW) * S * T::HC + (s_lo % T::TW) * S) * kPixB + choff;
      const char* x_hi = halo + ((s_hi / T::TW) * S * T::HC + (s_hi % T::TW) * S) * kPixB + choff;
#pragma unroll
      for (int j = 0; j < UPW; ++j) {
        const int u = wave + 4 * j;
        const int gr = u / Cf::CBS, cib = u - gr * Cf::CBS;
        if (u < U && c0 + gr * G < g.C) {  // (wave-uniform)
          bf16x8 dyf[Cf::CBS];
#pragma unroll
          for (int cb = 0; cb < Cf::CBS; ++cb)
            dyf[cb] = tr_frag(d_lo + (gr * G + cb * 16) * 2, d_hi + (gr * G + cb * 16) * 2);
          const int xc = (gr * G + cib * 16) * 2;
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const int toff = ((t / 3) * T::HC + t % 3) * kPixB + xc;
            const bf16x8 xf = tr_frag(x_lo + toff, x_hi + toff);
#pragma unroll
            for (int cb = 0; cb < Cf::CBS; ++cb)
              acc[j][t][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, dyf[cb], acc[j][t][cb], 0, 0, 0);
          }
        }
      }
    }
  }
  // the block's slab, [C][G][9] or (chl: the channels-last order of the parameter) [C][9][G]:
  // lane holds ci = 16 cib + 4 lg + r, co = 16 cb + li
  const int s_ci = chl ? 1 : 9, s_tap = chl ? G : 1;
  float* slab = ws + (long)blockIdx.x * g.C * G * 9;
#pragma unroll
  for (int j = 0; j < UPW; ++j) {
    const int u = wave + 4 * j;
    const int gr = u / Cf::CBS, cib = u - gr * Cf::CBS;
    if (u < U && c0 + gr * G < g.C) {
#pragma unroll
      for (int cb = 0; cb < Cf::CBS; ++cb) {
        const int co = cb * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ci = cib * 16 + 4 * lg + r;
          if (co < G && ci < G) {
            float* o = slab + (long)(c0 + gr * G + co) * G * 9 + ci * s_ci;
#pragma unroll
            for (int t = 0; t < 9; ++t) o[t * s_tap] = acc[j][t][cb][r];
          }
        }
      }
    }
  }
}

inline Gc3Geom gc3_geom(int N, int C, int ih, int iw, int oh, int ow, int th, int tw) {
  Gc3Geom g;
  const int nth = (oh + th - 1) / th, ntw = (ow + tw - 1) / tw;
  g.ftw = FastDiv((uint32_t)ntw);
  g.fth = FastDiv((uint32_t)nth);
  g.N = N; g.C = C; g.IH = ih; g.IW = iw; g.OH = oh; g.OW = ow;
  g.ntiles = (uint32_t)((long)N * nth * ntw);
  return g;
}

// f(G, S as integral constants) for the supported (G, s)
template <class F>
inline void dispatch_gc3(int G, int s, F&& f) {
  dispatch_int<8, 16, 24, 32, 40, 48, 56, 64>(G, [&](auto gg) {
    dispatch_int<1, 2>(s, [&](auto ss) { f(gg, ss); });
  });
}

}  // namespace

void gconv3_fwd(const void* x, const void* w, const float* shift, void* y, float* ws, float* ps,
                float* pss, int N, int H, int W, int C, int G, int s, hipStream_t st) {
  if ((long)N * H * W * C <= 0 || !gc3_supported(C, G, s)) return;
  const int Ho = gc3_out(H, s), Wo = gc3_out(W, s);
  const Gc3Geom g = gc3_geom(N, C, H, W, Ho, Wo, gc3_tile_h(s), gc3_tile_w(s));
  const int P = gc3_stat_rows(N, Ho, Wo, s);
  float* ws_q = ws == nullptr ? nullptr : ws + (long)P * C;
  const int cb = gc3_groups_per_block(G) * G;
  const dim3 grid(P, (C + cb - 1) / cb);
  dispatch_gc3(G, s, [&](auto gg, auto ss) {
    dispatch_bool(shift != nullptr, [&](auto stats) {
      hipLaunchKernelGGL((gconv3_fwd_kernel<decltype(gg)::value, decltype(ss)::value,
                                            decltype(stats)::value>),
                         grid, dim3(kGc3Threads), 0, st, (const __bf16*)x, (const __bf16*)w, shift,
                         (__bf16*)y, ws, ws_q, g);
    });
  });
  if (shift != nullptr) det_sum_rows(ws, ws_q, P, C, ps, pss, false, st);
}

void gconv3_dgrad(const void* dy, const void* w, const void* addend, void* dx, int N, int H, int W,
                  int C, int G, int s, hipStream_t st) {
  if ((long)N * H * W * C <= 0 || !gc3_supported(C, G, s)) return;
  const int Ho = gc3_out(H, s), Wo = gc3_out(W, s);
  const Gc3Geom g = s == 1 ? gc3_geom(N, C, H, W, H, W, gc3_tile_h(1), gc3_tile_w(1))
                           : gc3_geom(N, C, Ho, Wo, H, W, kGc3DgradTile, kGc3DgradTile);
  const int cb = gc3_groups_per_block(G) * G;
  const dim3 grid(std::min<uint32_t>(g.ntiles, kGc3MaxBlocks), (C + cb - 1) / cb);
  dispatch_gc3(G, s, [&](auto gg, auto ss) {
    constexpr int GG = decltype(gg)::value;
    dispatch_bool(addend != nullptr, [&](auto add) {
      constexpr bool ADD = decltype(add)::value;
      if constexpr (decltype(ss)::value == 1)
        hipLaunchKernelGGL((gconv3_dgrad_kernel<GG, ADD>), grid, dim3(kGc3Threads), 0, st,
                           (const __bf16*)dy, (const __bf16*)w, (const __bf16*)addend, (__bf16*)dx, g);
      else
        hipLaunchKernelGGL((gconv3_dgrad2_kernel<GG, ADD>), grid, dim3(kGc3Threads), 0, st,
                           (const __bf16*)dy, (const __bf16*)w, (const __bf16*)addend, (__bf16*)dx, g);
    });
  });
}

void gconv3_wgrad(const void* dy, const void* x, float* ws, float* dw, int N, int H, int W, int C,
                  int G, int s, bool channels_last, hipStream_t st) {
  if ((long)N * H * W * C <= 0 || !gc3_supported(C, G, s)) return;
  const int Ho = gc3_out(H, s), Wo = gc3_out(W, s);
  const Gc3Geom g = gc3_geom(N, C, H, W, Ho, Wo, gc3_tile_h(s), gc3_tile_w(s));
  const int P = gc3_wgrad_rows(N, Ho, Wo, C, G, s);
  const int cb = gc3_groups_per_block(G) * G;
  const dim3 grid(P, (C + cb - 1) / cb);
  dispatch_gc3(G, s, [&](auto gg, auto ss) {
    hipLaunchKernelGGL((gconv3_wgrad_kernel<decltype(gg)::value, decltype(ss)::value>), grid,
                       dim3(kGc3Threads), 0, st, (const __bf16*)dy, (const __bf16*)x, ws, g,
                       channels_last ? 1 : 0);
  });
  det_sum_rows(ws, nullptr, P, C * G * 9, dw, nullptr, true, st);
}

}  // namespace mipipe
