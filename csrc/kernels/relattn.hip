// MaxViT's partition attention for gfx950: head width 32, 49-token partitions of an NHWC token
// map in two compile-time modes, forward + backward, with a [169][H] relative-position table and
// the score scale as a launch argument (torchvision's MaxViT scales by C^-1/2 of the WHOLE
// channel count, not of the head width).
//
// Per (window, head): P = softmax(q·kᵀ·scale + table[rel(i, j)]), o = P·v.  The tile frame is
// wintile.hpp's at WS = 7 (Geo<7>, 49 live tokens padded to 64 through the E tile, fill_bias,
// ld_frags, the LDS images, the fixed-order table gradient); the arithmetic is winattn.hip's with
// the scale folded into the fp32 score tile as scale·log2e next to the bias add, and carried into
// dQ and dK where Swin carries its constant.  What is this file's own:
//
//   token addressing (part_window<GRID>): window w of a map with py = Hs/7, px = Ws/7 is
//     block  w = (b·py + wy)·px + wx,  token (y, x) -> row (b·Hs + wy·7 + y)·Ws + wx·7 + x
//     grid   w = (b·py + a)·px + b',   token (y, x) -> row (b·Hs + y·py + a)·Ws + x·px + b'
//   Neither mode has a shift, a region mask or border windows: no mask bits are built or applied.
//
//   grid-mode run order.  A token's head slice is 64 bytes and a qkv row at least 192, so two
//   windows never share a cache line: what can be shared is the DRAM page and the row buffer.  The
//   window index therefore runs b' fastest, then a: the kWinRun windows of a block's run, and the
//   kWinWaves windows its waves hold at one time, are ADJACENT token rows under every one of the
//   49 (gy, gx) positions, so a run reads 49 (or, across a row end, 98) contiguous stretches of
//   kWinRun·ld·2 bytes instead of 49·kWinRun scattered rows, and the same holds for the dqkv / o
//   stores.  The alternative orders (a fastest, or windows dealt round-robin to the runs) put
//   py·Ws rows between concurrently read tokens and were not taken.
#include "common.hpp"
#include "launchers.hpp"
#include "wintile.hpp"

namespace mipipe {
namespace relattn {

using namespace wintile;

constexpr int WS = 7;
constexpr int NT = Geo<WS>::NT, NREL = Geo<WS>::NREL, kEBytes = Geo<WS>::kEBytes;

struct Args : WinArgs {
  float scale, scale_log2;
};

// the rows of window w's tokens live_token(32*t + (lane & 31)); nwy = Hs / 7, nwx = Ws / 7
template <bool GRID>
__device__ __forceinline__ Win part_window(const WinArgs& a, int w, int lane) {
  const int c = w % a.nwx, t = w / a.nwx, r = t % a.nwy, b = t / a.nwy;
  Win g;
  g.lasty = g.lastx = false;  // never read
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    const int n = live_token<WS>(32 * tt + (lane & 31));
    const int y = n / WS, x = n % WS;
    const int gy = GRID ? y * a.nwy + r : r * WS + y;
    const int gx = GRID ? x * a.nwx + c : c * WS + x;
    g.row[tt] = ((long)b * a.Hs + gy) * a.Ws + gx;
  }
  return g;
}

// Lane = query n = 32*qt + r: p[sub][i] = softmax over keys 32*sub + acc_row(i, hl), normalised;
// mu / inv_l the column's max and 1 / sum (both 0 for a dead query)
__device__ __forceinline__ void probs_by_query(const bf16x8 (&kf)[2][2], const bf16x8 (&qf)[2],
                                               const float* Eq, float scale_log2, int hl,
                                               f32x16 (&p)[2], float& mu, float& inv_l) {
  float m = -INFINITY;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    p[sub] = mfma32(kf[sub][1], qf[1], mfma32(kf[sub][0], qf[0], zero16()));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float v = p[sub][i] * scale_log2 + Eq[32 * sub + acc_row(i, hl)];
      p[sub][i] = v;
      m = fmaxf(m, v);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32));
  mu = m == -INFINITY ? 0.f : m;
  float l = 0.f;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      p[sub][i] = exp2f(p[sub][i] - mu);
      l += p[sub][i];
    }
  l += __shfl_xor(l, 32);
  inv_l = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int i = 0; i < 16; ++i) p[sub][i] *= inv_l;
}

template <bool GRID>
__global__ __launch_bounds__(64 * kWinWaves) void relattn_fwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) char smem[kEBytes + kWinWaves * kImg];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5, r = lane & 31;
  const int h = blockIdx.x % a.H, run = blockIdx.x / a.H;
  float* E = reinterpret_cast<float*>(smem);
  char* vimg = smem + kEBytes + wave * kImg;
  fill_bias<WS>(E, a, h, tid, 64 * kWinWaves);
  __syncthreads();
  const long ld = 3l * a.H * D, ldo = (long)a.H * D;
  const __bf16* qb = a.qkv + h * D;
  const int ngroups = win_groups(a.nwin);
  for (int grp = run; grp < ngroups; grp += a.nruns)
    for (int w = grp * kWinRun + wave; w < min((grp + 1) * kWinRun, a.nwin); w += kWinWaves) {
      const Win g = part_window<GRID>(a, w, lane);
      bf16x8 qf[2][2], kf[2][2], vf[2][2];
      ld_frags(qb, g, ld, hl, qf);
      ld_frags(qb + ldo, g, ld, hl, kf);
      ld_frags(qb + 2 * ldo, g, ld, hl, vf);
      wave_lds_fence();  // the previous window's transposed reads are done
      st_image(vimg, vf, lane);
      wave_lds_fence();
      bf16x8 vt[2][2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) vt[sub][ks] = ld_tr(vimg, 32 * sub + 16 * ks, lane);
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const int qn = 32 * qt + r;
        f32x16 p[2];
        float mu, inv_l;
        probs_by_query(kf, qf[qt], E + min(qn, NT) * kEP, a.scale_log2, hl, p, mu, inv_l);
        f32x16 o = zero16();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) o = mfma32(vt[sub][ks], pack_acc(p[sub], ks), o);
        if (qn < NT) st_cols(a.o + g.row[qt] * ldo + h * D, o, 1.f, hl);
      }
    }
}

// LDS per wave: image X (K, then dO) | image Y (Q) | per-query max, 1/sum, δ
constexpr int kBwdWave = 2 * kImg + 3 * 64 * 4;

// Phase A (lane = query): Pᵀ, dPᵀ = V·dOᵀ, δ = Σ_k P∘dP, dSᵀ = P∘(dP-δ), dQᵀ = Kᵀ·dSᵀ·scale, the
// per-query (max, 1/sum, δ) to LDS.  Phase B (lane = key): P and dS again with a key per lane
// from those statistics, dVᵀ = dOᵀ·P, dKᵀ = Qᵀ·dS·scale.  dtable: the wave's fp32 sum of dSᵀ.
template <bool GRID>
__global__ __launch_bounds__(64 * kWinWaves) void relattn_bwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) char smem[kEBytes + kWinWaves * kBwdWave];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5, r = lane & 31;
  const int h = blockIdx.x % a.H, run = blockIdx.x / a.H;
  float* E = reinterpret_cast<float*>(smem);
  char* ximg = smem + kEBytes + wave * kBwdWave;
  char* yimg = ximg + kImg;
  float* stat = reinterpret_cast<float*>(yimg + kImg);  // [3][64]
  fill_bias<WS>(E, a, h, tid, 64 * kWinWaves);
  __syncthreads();
  const long ld = 3l * a.H * D, ldo = (long)a.H * D;
  const __bf16* qb = a.qkv + h * D;
  f32x16 dsum[2][2];  // Σ over this wave's windows of dSᵀ: [query tile][key tile]
#pragma unroll
  for (int i = 0; i < 4; ++i) dsum[i >> 1][i & 1] = zero16();
  const int ngroups = win_groups(a.nwin);
  for (int grp = run; grp < ngroups; grp += a.nruns)
    for (int w = grp * kWinRun + wave; w < min((grp + 1) * kWinRun, a.nwin); w += kWinWaves) {
      const Win g = part_window<GRID>(a, w, lane);
      bf16x8 qf[2][2], kf[2][2], vf[2][2], df[2][2];
      ld_frags(qb, g, ld, hl, qf);
      ld_frags(qb + ldo, g, ld, hl, kf);
      ld_frags(qb + 2 * ldo, g, ld, hl, vf);
      ld_frags(a.dout + h * D, g, ldo, hl, df);
      wave_lds_fence();
      st_image(ximg, kf, lane);
      st_image(yimg, qf, lane);
      wave_lds_fence();
      // ---- phase A: lane = query
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        __builtin_amdgcn_sched_barrier(0);
        const int qn = 32 * qt + r;
        f32x16 p[2];
        float mu, inv_l;
        probs_by_query(kf, qf[qt], E + min(qn, NT) * kEP, a.scale_log2, hl, p, mu, inv_l);
        f32x16 dp[2];
        float delta = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          dp[sub] = mfma32(vf[sub][1], df[qt][1], mfma32(vf[sub][0], df[qt][0], zero16()));
#pragma unroll
          for (int i = 0; i < 16; ++i) delta += p[sub][i] * dp[sub][i];
        }
        delta += __shfl_xor(delta, 32);
        f32x16 dq = zero16();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            p[sub][i] *= dp[sub][i] - delta;  // dSᵀ; exactly 0 for dead queries and keys (p = 0)
            dsum[qt][sub][i] += p[sub][i];
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            dq = mfma32(ld_tr(ximg, 32 * sub + 16 * ks, lane), pack_acc(p[sub], ks), dq);
        }
        if (qn < NT) st_cols(a.dqkv + g.row[qt] * ld + h * D, dq, a.scale, hl);
        if (hl == 0) {
          stat[qn] = mu;
          stat[64 + qn] = inv_l;
          stat[128 + qn] = delta;
        }
      }
      wave_lds_fence();  // phase A's reads of the K image are done, the statistics are written
      st_image(ximg, df, lane);
      wave_lds_fence();
      // ---- phase B: lane = key
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        __builtin_amdgcn_sched_barrier(0);
        const int kn = 32 * kt + r;
        f32x16 dv = zero16(), dk = zero16();
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
          __builtin_amdgcn_sched_barrier(0);
          f32x16 p = mfma32(qf[qs][1], kf[kt][1], mfma32(qf[qs][0], kf[kt][0], zero16()));
          f32x16 ds = mfma32(df[qs][1], vf[kt][1], mfma32(df[qs][0], vf[kt][0], zero16()));
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int qn = 32 * qs + acc_row(i, hl);
            const float v = p[i] * a.scale_log2 + E[min(qn, NT) * kEP + kn];
            p[i] = exp2f(v - stat[qn]) * stat[64 + qn];
            ds[i] = p[i] * (ds[i] - stat[128 + qn]);
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            dv = mfma32(ld_tr(ximg, 32 * qs + 16 * ks, lane), pack_acc(p, ks), dv);
            dk = mfma32(ld_tr(yimg, 32 * qs + 16 * ks, lane), pack_acc(ds, ks), dk);
          }
        }
        if (kn < NT) {
          __bf16* dst = a.dqkv + g.row[kt] * ld + ldo + h * D;
          st_cols(dst, dk, a.scale, hl);
          st_cols(dst + ldo, dv, 1.f, hl);
        }
      }
    }
  // ---- table gradient
  dsum_to_E<WS>(E, dsum, wave, lane);
  __syncthreads();
  if (tid < NREL) st_bias_partial<WS>(E, a, run, h, tid);
}

}  // namespace relattn

static relattn::Args relattn_args(const void* qkv, const float* table, int B, int Hs, int Ws,
                                  int H, float scale) {
  relattn::Args a{};
  wintile::win_geometry<relattn::WS>(a, qkv, table, B, Hs, Ws, H, 0, 0);
  a.scale = scale;
  a.scale_log2 = scale * wintile::kLog2e;
  return a;
}

void relattn_fwd(const void* qkv, const float* table, void* o, int B, int Hs, int Ws, int H,
                 bool grid, float scale, hipStream_t st) {
  relattn::Args a = relattn_args(qkv, table, B, Hs, Ws, H, scale);
  a.o = (__bf16*)o;
  const dim3 blocks(a.nruns * H), threads(64 * kWinWaves);
  if (grid) hipLaunchKernelGGL(relattn::relattn_fwd_kernel<true>, blocks, threads, 0, st, a);
  else hipLaunchKernelGGL(relattn::relattn_fwd_kernel<false>, blocks, threads, 0, st, a);
}

void relattn_bwd(const void* dout, const void* qkv, const float* table, void* dqkv,
                 float* partial, float* dtable, int B, int Hs, int Ws, int H, bool grid,
                 float scale, hipStream_t st) {
  relattn::Args a = relattn_args(qkv, table, B, Hs, Ws, H, scale);
  a.dout = (const __bf16*)dout;
  a.dqkv = (__bf16*)dqkv;
  a.partial = partial;
  const dim3 blocks(a.nruns * H), threads(64 * kWinWaves);
  if (grid) hipLaunchKernelGGL(relattn::relattn_bwd_kernel<true>, blocks, threads, 0, st, a);
  else hipLaunchKernelGGL(relattn::relattn_bwd_kernel<false>, blocks, threads, 0, st, a);
  det_sum_rows(partial, nullptr, a.nruns, relattn::NREL * H, dtable, nullptr, true, st);
}

}  // namespace mipipe
