// The frame the window-attention kernels share (winattn.hip: Swin, 7x7 windows, scaled dot-product
// scores; winattn8.hip: Swin V2, 8x8 windows, cosine scores), templated on the window side WS,
// and the 64-token x 32-wide tile pieces under it.  The score / softmax / backward arithmetic is
// each kernel file's own.
//
// Frame: qkv [B*Hs*Ws][3*H*32] bf16 (q | k | v, head-major, rows in NHWC token order), o
// [B*Hs*Ws][H*32], dqkv like qkv, bias fp32 [(2WS-1)^2][H].  The token at (wy*WS+y, wx*WS+x) of
// the SHIFTED map is row ((wy*WS+y+sy) mod Hs, (wx*WS+x+sx) mod Ws) of qkv / o / dqkv: roll,
// window partition, reverse and un-roll are address arithmetic only (window()).  The mask is -100
// between tokens of different shift regions (boundary at WS - shift per axis): bits per lane,
// computed once per block (lane_masks()), applied in the windows on the wrapped border.
//
// One wave owns one (window, head) at a time: a whole window-head is NT = WS*WS <= 64 tokens x
// 32, so scores, softmax, P·V and the full backward live in one wave's registers: no online
// softmax, no lse, no K/V streaming, no dQ atomics.  A block = kWinWaves waves of ONE head
// walking groups of kWinRun windows (grid-strided past kWinMaxRuns group slots).  Per block, once:
// the head's bias expanded to E[query][key] in LDS, log2 domain (fill_bias()).
//
// NT < 64 (7x7: 49 live tokens in the 64-row tile): the dead lanes address the window's last
// token (live_token()), E has -inf dead columns and one all -inf row that every dead query reads,
// so padding drops out of every sum as an exact zero, and nothing is stored for a dead token.
// At NT == 64 all of that folds away.
//
// Bias gradient: a lane's accumulator registers hold the same (query, key) for every window, so a
// wave sums dSᵀ over its windows in fp32 registers; at the end the block's waves add their sums in
// wave order into the (reused) E tile (dsum_to_E()), one thread per table entry adds its
// diagonal's entries in index order into the partial row of (group slot, head)
// (st_bias_partial()), and det_sum_rows adds the partial rows in order into the gradient (+=).
// No float atomics: the same bits on every launch in every mode.
//
// Tile pieces: tile32.hpp's 32x32x16 bf16 MFMA in "swapped" orientation (a lane owns a column,
// so a softmax row is in-lane) with an accumulator packed as the next product's B operand, and
// here the [64][32] bf16 LDS images with their transposed reads.
#pragma once
#include "common.hpp"
#include "launchers.hpp"
#include "tile32.hpp"

namespace mipipe {
namespace wintile {

using namespace tile32;

constexpr int D = 32;                 // head width
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kMaskLog2 = -100.f * kLog2e;
constexpr int kPitch = 80;            // bytes per row of a [64][32] bf16 LDS image (16-B aligned)
constexpr int kImg = 64 * kPitch;
constexpr int kEP = 65;               // floats per row of E (conflict-free along both axes)

template <int WS>
struct Geo {
  static constexpr int NT = WS * WS;  // tokens per window
  static constexpr int NREL = (2 * WS - 1) * (2 * WS - 1);
  static constexpr int kERows = NT < 64 ? NT + 1 : NT;  // + one all -inf row for the dead queries
  static constexpr int kEBytes = (kERows * kEP * 4 + 15) / 16 * 16;
  static_assert(NT <= 64 && NREL <= 64 * kWinWaves, "tile geometry");
};

// What both kernels' Args start with; the geometry part is filled by win_geometry().
struct WinArgs {
  const __bf16* qkv;
  const __bf16* dout;   // backward
  __bf16* o;            // forward
  __bf16* dqkv;         // backward
  const float* bias;    // [NREL][H]
  float* partial;       // backward: [nruns][NREL * H]
  int Hs, Ws, H, sy, sx, nwy, nwx;
  int nwin;             // B * nwy * nwx
  int nruns;            // group slots = gridDim.x / H
};

__host__ __device__ __forceinline__ int win_groups(int nwin) {
  return (nwin + kWinRun - 1) / kWinRun;
}

template <int WS>
inline void win_geometry(WinArgs& a, const void* qkv, const float* bias, int B, int Hs, int Ws,
                         int H, int sy, int sx) {
  a.qkv = (const __bf16*)qkv;
  a.bias = bias;
  a.Hs = Hs; a.Ws = Ws; a.H = H; a.sy = sy; a.sx = sx;
  a.nwy = Hs / WS;
  a.nwx = Ws / WS;
  a.nwin = B * a.nwy * a.nwx;
  a.nruns = winattn_runs(a.nwin);
}

// tile row n -> the token it addresses: itself, or the window's last token for a dead row
template <int WS>
__device__ __forceinline__ int live_token(int n) {
  return Geo<WS>::NT < 64 ? min(n, Geo<WS>::NT - 1) : n;
}

// E[min(q, NT)][k] = bias[rel(q, k)][h] * log2e for live (q, k), -inf for dead ones, with
// rel(q, k) = (yq-yk+WS-1)*(2WS-1) + (xq-xk+WS-1)
template <int WS>
__device__ __forceinline__ void fill_bias(float* E, const WinArgs& a, int h, int tid, int nthr) {
  constexpr int NT = Geo<WS>::NT;
  for (int idx = tid; idx < Geo<WS>::kERows * 64; idx += nthr) {
    const int q = idx >> 6, k = idx & 63;
    float v = -INFINITY;
    if (NT == 64 || (q < NT && k < NT)) {
      const int rel = (q / WS - k / WS + WS - 1) * (2 * WS - 1) + (q % WS - k % WS + WS - 1);
      v = a.bias[(long)rel * a.H + h] * kLog2e;
    }
    E[q * kEP + k] = v;
  }
}

// The lane's part of the region mask, the same bits in both orientations (the relation is
// symmetric): bit 16*t + i of my / mx <-> tokens n = 32*tile + (lane & 31) and 32*t +
// acc_row(i, hl) lie on different sides of the axis' shift boundary (WS - shift).
template <int WS>
__device__ __forceinline__ void lane_masks(int tile, int lane, int sy, int sx, uint32_t& my,
                                           uint32_t& mx) {
  const int n = live_token<WS>(32 * tile + (lane & 31)), hl = lane >> 5;
  const bool ny = n / WS < WS - sy, nx = n % WS < WS - sx;
  my = mx = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = live_token<WS>(32 * t + acc_row(i, hl));
      my |= (uint32_t)((m / WS < WS - sy) != ny) << (16 * t + i);
      mx |= (uint32_t)((m % WS < WS - sx) != nx) << (16 * t + i);
    }
}

struct Win {
  long row[2];        // qkv / o row of token live_token(32*t + (lane & 31))
  bool lasty, lastx;  // the window touches the wrapped border of a shifted axis
};
template <int WS>
__device__ __forceinline__ Win window(const WinArgs& a, int w, int lane) {
  const int wx = w % a.nwx, t = w / a.nwx, wy = t % a.nwy, b = t / a.nwy;
  Win g;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int n = live_token<WS>(32 * tt + (lane & 31));
    int gy = wy * WS + n / WS + a.sy, gx = wx * WS + n % WS + a.sx;
    gy -= gy >= a.Hs ? a.Hs : 0;
    gx -= gx >= a.Ws ? a.Ws : 0;
    g.row[tt] = ((long)b * a.Hs + gy) * a.Ws + gx;
  }
  g.lasty = a.sy != 0 && wy == a.nwy - 1;
  g.lastx = a.sx != 0 && wx == a.nwx - 1;
  return g;
}

// the two 16-byte k-steps of token rows' head slice as MFMA operands (row = lane & 31)
__device__ __forceinline__ void ld_frags(const __bf16* base, const Win& g, long ld, int hl,
                                         bf16x8 (&f)[2][2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int st = 0; st < 2; ++st)
      f[t][st] = *reinterpret_cast<const bf16x8*>(base + g.row[t] * ld + 16 * st + 8 * hl);
}

// Bias gradient, first half: dsum[query tile][key tile] (lane = query 32*qt + (lane & 31), regs =
// keys) of the block's waves added in wave order into E.  Ends without a barrier.
template <int WS>
__device__ __forceinline__ void dsum_to_E(float* E, const f32x16 (&dsum)[2][2], int wave,
                                          int lane) {
  constexpr int NT = Geo<WS>::NT;
  const int hl = lane >> 5, r = lane & 31;
  for (int wv = 0; wv < kWinWaves; ++wv) {
    __syncthreads();
    if (wave != wv) continue;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int qn = 32 * qt + r, kn = 32 * sub + acc_row(i, hl);
          if (NT == 64 || qn < NT) {
            float* e = E + qn * kEP + kn;
            *e = wv == 0 ? dsum[qt][sub][i] : *e + dsum[qt][sub][i];
          }
        }
  }
}
// Second half, after a barrier: thread tid < NREL adds table entry tid's diagonal of E, its
// (query, key) pairs in index order, into the partial row of (group slot run, head h).
template <int WS>
__device__ __forceinline__ void st_bias_partial(const float* E, const WinArgs& a, int run, int h,
                                                int tid) {
  constexpr int NREL = Geo<WS>::NREL;
  const int dy = tid / (2 * WS - 1) - (WS - 1), dx = tid % (2 * WS - 1) - (WS - 1);
  float acc = 0.f;
  for (int yq = max(0, dy); yq <= min(WS - 1, WS - 1 + dy); ++yq)
    for (int xq = max(0, dx); xq <= min(WS - 1, WS - 1 + dx); ++xq)
      acc += E[(yq * WS + xq) * kEP + (yq - dy) * WS + (xq - dx)];
  a.partial[(long)run * NREL * a.H + (long)tid * a.H + h] = acc;
}

// A operand holding Tᵀ of a row-major [64][32] image T, k (row) order of pack_acc: element j of
// lane half h <-> row r0 + 8(j>>2) + 4h + (j&3); the lane's column is lane & 31.
__device__ __forceinline__ bf16x8 ld_tr(const char* img, uint32_t r0, int lane) {
  const uint32_t hl = lane >> 5, li = lane & 15, q = li >> 2, p = li & 3;
  const char* a0 = img + (r0 + 4 * hl + q) * kPitch + (16 * ((lane >> 4) & 1) + 4 * p) * 2;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(a0 + 8 * kPitch));
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
// this wave's LDS accesses so far have completed; nothing moves across (wave-private images)
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// the lane's operand fragments (row = 32t + (lane & 31), elements 16st + 8hl ..) -> the image
__device__ __forceinline__ void st_image(char* img, const bf16x8 (&f)[2][2], int lane) {
  const int r = lane & 31, hl = lane >> 5;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int st = 0; st < 2; ++st)
      *reinterpret_cast<bf16x8*>(img + (32 * t + r) * kPitch + (16 * st + 8 * hl) * 2) = f[t][st];
}
// accumulator (lane = token column, regs = d rows) -> 8-byte pieces of the token's head slice
__device__ __forceinline__ void st_cols(__bf16* dst, const f32x16& x, float s, int hl) {
#pragma unroll
  for (int ig = 0; ig < 4; ++ig)
    *reinterpret_cast<uint2*>(dst + 8 * ig + 4 * hl) =
        make_uint2(pack2(x[4 * ig] * s, x[4 * ig + 1] * s),
                   pack2(x[4 * ig + 2] * s, x[4 * ig + 3] * s));
}

}  // namespace wintile
}  // namespace mipipe
