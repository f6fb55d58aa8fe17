// Swin's shifted-window attention for gfx950: head width 32, 7x7 windows, forward + backward,
// and the PatchMerging permutation.
//
// Layout, the roll / window / mask addressing, the block's walk over the windows and the
// bias-table gradient's fixed-order sum are wintile.hpp's frame at WS = 7 (49 live tokens padded
// to 64 inside the tile); table [169][H] fp32 is the master relative_position_bias_table, read as
// it stands.  Per (window, head): P = softmax(q·kᵀ·scale + table[rel(i,j)] + mask(i,j)), o = P·v.
//
//   forward   Xᵀ = K·Qᵀ on mfma_f32_32x32x16_bf16 (2x2 tiles x 2 k-steps), K / Q fragments loaded
//             straight from global memory into the operand registers (16-byte loads, no LDS); a
//             lane owns a query column, so max / sum are in-lane + one cross-half exchange.
//             Oᵀ = Vᵀ·P with the bf16-converted accumulator as the B operand and Vᵀ read from a
//             per-wave LDS image by ds_read_b64_tr_b16.
//   backward  phase A (lane = query): recompute Pᵀ, dPᵀ = V·dOᵀ, δ = Σ_k P∘dP (= rowsum(dO∘O),
//             from fp32 values, O is not read), dSᵀ = P∘(dP-δ), dQᵀ = Kᵀ·dSᵀ; the per-query
//             (max, 1/sum, δ) go to LDS.  Phase B (lane = key): the same two products with the
//             operands swapped give P and dS with a key per lane (the statistics come from LDS,
//             so no cross-lane reduction), then dVᵀ = dOᵀ·P and dKᵀ = Qᵀ·dS.  Every product uses
//             "accumulator as the next B operand"; Kᵀ, Qᵀ, dOᵀ come from LDS images by
//             transposed reads.  dqkv is stored at the same rolled addresses.
//   dtable    the wave sums dSᵀ over its windows in fp32 registers (dsum); the frame does the rest.
#include "common.hpp"
#include "launchers.hpp"
#include "wintile.hpp"

namespace mipipe {
namespace winattn {

using namespace wintile;

constexpr int WS = 7;  // window side
constexpr int NT = Geo<WS>::NT, NREL = Geo<WS>::NREL, kEBytes = Geo<WS>::kEBytes;

struct Args : WinArgs {
  float scale, scale_log2;
};

// Lane = query n = 32*qt + r: p[sub][i] = softmax over keys 32*sub + acc_row(i, hl), normalised;
// mu / inv_l the column's max (0 for a dead query) and 1 / sum (0 for a dead query).
__device__ __forceinline__ void probs_by_query(const bf16x8 (&kf)[2][2], const bf16x8 (&qf)[2],
                                               const float* Eq, uint32_t mbits, float scale_log2,
                                               int hl, f32x16 (&p)[2], float& mu, float& inv_l) {
  float m = -INFINITY;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    p[sub] = mfma32(kf[sub][1], qf[1], mfma32(kf[sub][0], qf[0], zero16()));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = p[sub][i] * scale_log2 + Eq[32 * sub + acc_row(i, hl)];
      v += (mbits >> (16 * sub + i)) & 1u ? kMaskLog2 : 0.f;
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

__global__ __launch_bounds__(64 * kWinWaves) void winattn_fwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) char smem[kEBytes + kWinWaves * kImg];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5, r = lane & 31;
  const int h = blockIdx.x % a.H, run = blockIdx.x / a.H;
  float* E = reinterpret_cast<float*>(smem);
  char* vimg = smem + kEBytes + wave * kImg;
  fill_bias<WS>(E, a, h, tid, 64 * kWinWaves);
  uint32_t my[2], mx[2];
  lane_masks<WS>(0, lane, a.sy, a.sx, my[0], mx[0]);
  lane_masks<WS>(1, lane, a.sy, a.sx, my[1], mx[1]);
  __syncthreads();
  const long ld = 3l * a.H * D, ldo = (long)a.H * D;
  const __bf16* qb = a.qkv + h * D;
  const int ngroups = win_groups(a.nwin);
  for (int grp = run; grp < ngroups; grp += a.nruns)
    for (int w = grp * kWinRun + wave; w < min((grp + 1) * kWinRun, a.nwin); w += kWinWaves) {
      const Win g = window<WS>(a, w, lane);
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
        const uint32_t mb = (g.lasty ? my[qt] : 0u) | (g.lastx ? mx[qt] : 0u);
        f32x16 p[2];
        float mu, inv_l;
        probs_by_query(kf, qf[qt], E + min(qn, NT) * kEP, mb, a.scale_log2, hl, p, mu, inv_l);
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

__global__ __launch_bounds__(64 * kWinWaves) void winattn_bwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) char smem[kEBytes + kWinWaves * kBwdWave];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5, r = lane & 31;
  const int h = blockIdx.x % a.H, run = blockIdx.x / a.H;
  float* E = reinterpret_cast<float*>(smem);
  char* ximg = smem + kEBytes + wave * kBwdWave;
  char* yimg = ximg + kImg;
  float* stat = reinterpret_cast<float*>(yimg + kImg);  // [3][64]
  fill_bias<WS>(E, a, h, tid, 64 * kWinWaves);
  uint32_t my[2], mx[2];
  lane_masks<WS>(0, lane, a.sy, a.sx, my[0], mx[0]);
  lane_masks<WS>(1, lane, a.sy, a.sx, my[1], mx[1]);
  __syncthreads();
  const long ld = 3l * a.H * D, ldo = (long)a.H * D;
  const __bf16* qb = a.qkv + h * D;
  f32x16 dsum[2][2];  // Σ over this wave's windows of dSᵀ: [query tile][key tile]
#pragma unroll
  for (int i = 0; i < 4; ++i) dsum[i >> 1][i & 1] = zero16();
  const int ngroups = win_groups(a.nwin);
  for (int grp = run; grp < ngroups; grp += a.nruns)
    for (int w = grp * kWinRun + wave; w < min((grp + 1) * kWinRun, a.nwin); w += kWinWaves) {
      const Win g = window<WS>(a, w, lane);
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
        const uint32_t mb = (g.lasty ? my[qt] : 0u) | (g.lastx ? mx[qt] : 0u);
        f32x16 p[2];
        float mu, inv_l;
        probs_by_query(kf, qf[qt], E + min(qn, NT) * kEP, mb, a.scale_log2, hl, p, mu, inv_l);
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
        const uint32_t mb = (g.lasty ? my[kt] : 0u) | (g.lastx ? mx[kt] : 0u);
        f32x16 dv = zero16(), dk = zero16();
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
          __builtin_amdgcn_sched_barrier(0);
          f32x16 p = mfma32(qf[qs][1], kf[kt][1], mfma32(qf[qs][0], kf[kt][0], zero16()));
          f32x16 ds = mfma32(df[qs][1], vf[kt][1], mfma32(df[qs][0], vf[kt][0], zero16()));
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int qn = 32 * qs + acc_row(i, hl);
            float v = p[i] * a.scale_log2 + E[min(qn, NT) * kEP + kn];
            v += (mb >> (16 * qs + i)) & 1u ? kMaskLog2 : 0.f;
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
  // ---- bias-table gradient
  dsum_to_E<WS>(E, dsum, wave, lane);
  __syncthreads();
  if (tid < NREL) st_bias_partial<WS>(E, a, run, h, tid);
}

// ------------------------------------------------------------------------------ patch_merge
// One item = 8 channels.  Forward: output item o of row (b, i, j), column group g, channels c8
// <- x[b, 2i + (g & 1), 2j + (g >> 1), c8].  Backward: dx item of (b, y, x, c8) <- dy row
// (b, y / 2, x / 2), group (y & 1) + 2 (x & 1).  Stores in output order, one owner per element.
template <bool BWD>
__global__ __launch_bounds__(256) void patch_merge_kernel(const uint4* __restrict__ in,
                                                          uint4* __restrict__ out, uint32_t items,
                                                          FastDiv fC8, FastDiv fW, FastDiv fH,
                                                          uint32_t Ws) {
  for (uint32_t o = blockIdx.x * 256 + threadIdx.x; o < items; o += gridDim.x * 256) {
    uint32_t t = fC8.div(o);
    const uint32_t c8 = o - t * fC8.d;
    uint32_t src;
    if (BWD) {  // fW = Ws, fH = Hs: o indexes dx
      const uint32_t u = fW.div(t), x = t - u * fW.d;
      const uint32_t b = fH.div(u), y = u - b * fH.d;
      const uint32_t row = (b * (fH.d >> 1) + (y >> 1)) * (Ws >> 1) + (x >> 1);
      src = (row * 4 + (y & 1) + 2 * (x & 1)) * fC8.d + c8;
    } else {  // fW = Ws / 2, fH = Hs / 2: o indexes the merged rows
      const uint32_t g = t & 3;
      t >>= 2;
      const uint32_t u = fW.div(t), j = t - u * fW.d;
      const uint32_t b = fH.div(u), i = u - b * fH.d;
      src = ((b * (2 * fH.d) + 2 * i + (g & 1)) * Ws + 2 * j + (g >> 1)) * fC8.d + c8;
    }
    out[o] = in[src];
  }
}

}  // namespace winattn

int winattn_runs(long nwin) {
  const long groups = (nwin + kWinRun - 1) / kWinRun;
  return (int)std::max<long>(1, std::min<long>(groups, kWinMaxRuns));
}

static winattn::Args winattn_args(const void* qkv, const float* table, int B, int Hs, int Ws,
                                  int H, int sy, int sx) {
  winattn::Args a{};
  wintile::win_geometry<winattn::WS>(a, qkv, table, B, Hs, Ws, H, sy, sx);
  a.scale = 0.17677669529663687f;  // 32^-1/2
  a.scale_log2 = a.scale * wintile::kLog2e;
  return a;
}

void winattn_fwd(const void* qkv, const float* table, void* o, int B, int Hs, int Ws, int H,
                 int sy, int sx, hipStream_t st) {
  winattn::Args a = winattn_args(qkv, table, B, Hs, Ws, H, sy, sx);
  a.o = (__bf16*)o;
  hipLaunchKernelGGL(winattn::winattn_fwd_kernel, dim3(a.nruns * H), dim3(64 * kWinWaves), 0, st,
                     a);
}

void winattn_bwd(const void* dout, const void* qkv, const float* table, void* dqkv,
                 float* partial, float* dtable, int B, int Hs, int Ws, int H, int sy, int sx,
                 hipStream_t st) {
  winattn::Args a = winattn_args(qkv, table, B, Hs, Ws, H, sy, sx);
  a.dout = (const __bf16*)dout;
  a.dqkv = (__bf16*)dqkv;
  a.partial = partial;
  hipLaunchKernelGGL(winattn::winattn_bwd_kernel, dim3(a.nruns * H), dim3(64 * kWinWaves), 0, st,
                     a);
  det_sum_rows(partial, nullptr, a.nruns, winattn::NREL * H, dtable, nullptr, true, st);
}

void patch_merge(const void* in, void* out, int B, int Hs, int Ws, int C, bool bwd,
                 hipStream_t st) {
  const long n = (long)B * Hs * Ws * C;
  if (n <= 0) return;
  const uint32_t items = (uint32_t)(n / 8);
  const FastDiv fC8((uint32_t)C / 8);
  const int grid = grid1d(items, 1, 4096);
  if (bwd)
    hipLaunchKernelGGL(winattn::patch_merge_kernel<true>, dim3(grid), dim3(256), 0, st,
                       (const uint4*)in, (uint4*)out, items, fC8, FastDiv((uint32_t)Ws),
                       FastDiv((uint32_t)Hs), (uint32_t)Ws);
  else
    hipLaunchKernelGGL(winattn::patch_merge_kernel<false>, dim3(grid), dim3(256), 0, st,
                       (const uint4*)in, (uint4*)out, items, fC8, FastDiv((uint32_t)Ws / 2),
                       FastDiv((uint32_t)Hs / 2), (uint32_t)Ws);
}

}  // namespace mipipe
