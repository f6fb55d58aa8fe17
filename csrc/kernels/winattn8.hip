// Swin V2's shifted-window cosine attention for gfx950: head width 32, 8x8 windows, forward +
// backward.
//
// Layout, the roll / window / mask addressing, the block's walk over the windows and the bias
// gradient's fixed-order sum are wintile.hpp's frame at WS = 8: 64 live tokens fill the tile, so
// there are no clamped rows and no -inf padding, and E is [64][64] (+1 pitch).  bias [225][H]
// fp32 is the finished continuous-position bias 16·sigmoid(cpb_mlp(coords)); logit_scale [H] fp32
// the master parameter as it stands.  Per (window, head): q̂ = q / max(‖q‖, 1e-12), k̂ likewise,
// τ = exp(min(logit_scale, ln 100)), P = softmax(τ·q̂k̂ᵀ + bias[rel(i,j)] + mask(i,j)), o = P·v.
//
// Every product runs on mfma_f32_32x32x16_bf16 in swapped orientation with the accumulator as the
// next B operand, as in winattn.hip; what the cosine scores change:
//   * q̂ / k̂ are never formed (no second bf16 rounding): the MFMAs run on the raw q, k and the
//     fp32 score tile is scaled by rq_i·rk_j·τ.  rq, rk = 1 / max(‖·‖, eps) come from an fp32 sum
//     of squares of the loaded fragments (16 elements in-lane + one cross-half exchange); the
//     factor of the tile's register axis is read from a per-wave LDS vector.
//   * backward, with c = the cosines, G_ij = dS_ij·τ·rq_i·rk_j, a_i = Σ_j dS_ij·τc_ij and
//     b_j = Σ_i dS_ij·τc_ij:  dq_i = Σ_j G_ij k_j - q_i·rq_i²·a_i,  dk_j = Σ_i G_ij q_i -
//     k_j·rk_j²·b_j  (the projections of the two normalisations; they vanish below eps, as
//     clamp's gradient does).  The register-axis factor of G goes into the B operand before it
//     is rounded, the lane-axis factor is applied to the fp32 result.  a_i is an in-lane row sum
//     of phase A (lane = query): the raw scores are recomputed by two more MFMAs once dS is
//     known instead of being held in 32 registers; b_j is one of phase B (lane = key).  K, Q and
//     dO keep an LDS image each for the whole window: the transposed operands and the rows of
//     the projection terms (in the accumulator's d order) are read from them.
//   * dlogit_scale[h] = Σ a_i (0 when logit_scale[h] > ln 100: clamp's gradient): a lane sums
//     its queries' a_i over the wave's windows, then a fixed butterfly over the lanes, the
//     block's waves in wave order, one entry per (group slot, head); det_sum_rows adds the
//     partial rows of both gradients in order (+=).  No float atomics anywhere.
#include "common.hpp"
#include "launchers.hpp"
#include "wintile.hpp"

namespace mipipe {
namespace winattn8 {

using namespace wintile;

constexpr int WS = 8;  // window side
constexpr int NT = Geo<WS>::NT, NREL = Geo<WS>::NREL, kEBytes = Geo<WS>::kEBytes;
constexpr float kLn100 = 4.605170185988092f;
constexpr float kEps = 1e-12f;  // F.normalize's
static_assert(NT == 64 && NREL < 64 * kWinWaves, "a full tile, and a thread past the table's");

struct Args : WinArgs {
  const float* logit_scale;  // [H]
  float* partial_ls;         // backward: [nruns][H]
};

// rn[t] = 1 / max(‖row 32t + (lane & 31)‖, eps): the lane's 16 elements in fp32, then the other
// half-wave's 16 (a commutative add: both halves hold the same bits)
__device__ __forceinline__ void inv_norms(const bf16x8 (&f)[2][2], float (&rn)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    float ss = 0.f;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = (float)f[t][st][j];
        ss += v * v;
      }
    ss += __shfl_xor(ss, 32);
    rn[t] = 1.f / fmaxf(sqrtf(ss), kEps);
  }
}
// rn² where the norm is above eps, 0 where the clamp holds (the projection term's factor)
__device__ __forceinline__ float proj_factor(float rn) { return rn < 1.f / kEps ? rn * rn : 0.f; }

// Lane = query n = 32*qt + r: p[sub][i] = softmax over keys 32*sub + acc_row(i, hl), normalised,
// of x·col·rkL[key] + E + mask in the log2 domain (col = rq·τ·log2e of the lane's query);
// mu / inv_l the column's max and 1 / sum.
__device__ __forceinline__ void probs_by_query(const bf16x8 (&kf)[2][2], const bf16x8 (&qf)[2],
                                               const float* Eq, const float* rkL, uint32_t mbits,
                                               float col, int hl, f32x16 (&p)[2], float& mu,
                                               float& inv_l) {
  float m = -INFINITY;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub) {
    p[sub] = mfma32(kf[sub][1], qf[1], mfma32(kf[sub][0], qf[0], zero16()));
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int kn = 32 * sub + acc_row(i, hl);
      float v = p[sub][i] * (col * rkL[kn]) + Eq[kn];
      v += (mbits >> (16 * sub + i)) & 1u ? kMaskLog2 : 0.f;
      p[sub][i] = v;
      m = fmaxf(m, v);
    }
  }
  mu = fmaxf(m, __shfl_xor(m, 32));
  float l = 0.f;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      p[sub][i] = exp2f(p[sub][i] - mu);
      l += p[sub][i];
    }
  l += __shfl_xor(l, 32);
  inv_l = 1.f / l;
#pragma unroll
  for (int sub = 0; sub < 2; ++sub)
#pragma unroll
    for (int i = 0; i < 16; ++i) p[sub][i] *= inv_l;
}

// x·s - row·c -> the token's head slice: accumulator x (lane = token column, regs = d rows),
// row = the token's 32 bf16 of an LDS image (read in the accumulator's d order)
__device__ __forceinline__ void st_cols_proj(__bf16* dst, const f32x16& x, float s,
                                             const char* row, float c, int hl) {
#pragma unroll
  for (int ig = 0; ig < 4; ++ig) {
    const uint2 u = *reinterpret_cast<const uint2*>(row + (8 * ig + 4 * hl) * 2);
    const float f0 = __uint_as_float(u.x << 16), f1 = __uint_as_float(u.x & 0xffff0000u);
    const float f2 = __uint_as_float(u.y << 16), f3 = __uint_as_float(u.y & 0xffff0000u);
    *reinterpret_cast<uint2*>(dst + 8 * ig + 4 * hl) =
        make_uint2(pack2(x[4 * ig] * s - f0 * c, x[4 * ig + 1] * s - f1 * c),
                   pack2(x[4 * ig + 2] * s - f2 * c, x[4 * ig + 3] * s - f3 * c));
  }
}

__device__ __forceinline__ float temperature(const Args& a, int h) {
  return expf(fminf(a.logit_scale[h], kLn100));
}

// LDS per wave, forward: image V | rk[64]
constexpr int kFwdWave = kImg + 64 * 4;

__global__ __launch_bounds__(64 * kWinWaves) void winattn8_fwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) char smem[kEBytes + kWinWaves * kFwdWave];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5, r = lane & 31;
  const int h = blockIdx.x % a.H, run = blockIdx.x / a.H;
  float* E = reinterpret_cast<float*>(smem);
  char* vimg = smem + kEBytes + wave * kFwdWave;
  float* rkL = reinterpret_cast<float*>(vimg + kImg);
  fill_bias<WS>(E, a, h, tid, 64 * kWinWaves);
  const float tau_log2 = temperature(a, h) * kLog2e;
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
      float rq[2], rk[2];
      inv_norms(qf, rq);
      inv_norms(kf, rk);
      wave_lds_fence();  // the previous window's reads of the image and of rk are done
      st_image(vimg, vf, lane);
      rkL[lane] = hl ? rk[1] : rk[0];
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
        probs_by_query(kf, qf[qt], E + qn * kEP, rkL, mb, rq[qt] * tau_log2, hl, p, mu, inv_l);
        f32x16 o = zero16();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) o = mfma32(vt[sub][ks], pack_acc(p[sub], ks), o);
        st_cols(a.o + g.row[qt] * ldo + h * D, o, 1.f, hl);
      }
    }
}

// LDS per wave, backward: images K | Q | dO | per-query max, 1/sum, δ, rq | per-key rk
constexpr int kBwdWave = 3 * kImg + 5 * 64 * 4;

__global__ __launch_bounds__(64 * kWinWaves) void winattn8_bwd_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) char smem[kEBytes + kWinWaves * kBwdWave];
  __shared__ float red[kWinWaves];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hl = lane >> 5, r = lane & 31;
  const int h = blockIdx.x % a.H, run = blockIdx.x / a.H;
  float* E = reinterpret_cast<float*>(smem);
  char* kimg = smem + kEBytes + wave * kBwdWave;
  char* qimg = kimg + kImg;
  char* dimg = qimg + kImg;
  float* stat = reinterpret_cast<float*>(dimg + kImg);  // [4][64] by query
  float* rkL = stat + 4 * 64;                           // [64] by key
  fill_bias<WS>(E, a, h, tid, 64 * kWinWaves);
  const float tau = temperature(a, h);
  uint32_t my[2], mx[2];
  lane_masks<WS>(0, lane, a.sy, a.sx, my[0], mx[0]);
  lane_masks<WS>(1, lane, a.sy, a.sx, my[1], mx[1]);
  __syncthreads();
  const long ld = 3l * a.H * D, ldo = (long)a.H * D;
  const __bf16* qb = a.qkv + h * D;
  f32x16 dsum[2][2];  // Σ over this wave's windows of dSᵀ: [query tile][key tile]
#pragma unroll
  for (int i = 0; i < 4; ++i) dsum[i >> 1][i & 1] = zero16();
  float lsum = 0.f;   // Σ over this wave's windows of a_i of the lane's two queries
  const int ngroups = win_groups(a.nwin);
  for (int grp = run; grp < ngroups; grp += a.nruns)
    for (int w = grp * kWinRun + wave; w < min((grp + 1) * kWinRun, a.nwin); w += kWinWaves) {
      const Win g = window<WS>(a, w, lane);
      bf16x8 qf[2][2], kf[2][2], vf[2][2], df[2][2];
      ld_frags(qb, g, ld, hl, qf);
      ld_frags(qb + ldo, g, ld, hl, kf);
      ld_frags(qb + 2 * ldo, g, ld, hl, vf);
      ld_frags(a.dout + h * D, g, ldo, hl, df);
      float rq[2], rk[2];
      inv_norms(qf, rq);
      inv_norms(kf, rk);
      wave_lds_fence();  // the previous window's reads are done
      st_image(kimg, kf, lane);
      st_image(qimg, qf, lane);
      st_image(dimg, df, lane);
      rkL[lane] = hl ? rk[1] : rk[0];
      stat[192 + lane] = hl ? rq[1] : rq[0];
      wave_lds_fence();
      // ---- phase A: lane = query
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        __builtin_amdgcn_sched_barrier(0);
        const int qn = 32 * qt + r;
        const uint32_t mb = (g.lasty ? my[qt] : 0u) | (g.lastx ? mx[qt] : 0u);
        const float rqt = rq[qt] * tau;
        f32x16 p[2];
        float mu, inv_l;
        probs_by_query(kf, qf[qt], E + qn * kEP, rkL, mb, rqt * kLog2e, hl, p, mu, inv_l);
        f32x16 dp[2];
        float delta = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          dp[sub] = mfma32(vf[sub][1], df[qt][1], mfma32(vf[sub][0], df[qt][0], zero16()));
#pragma unroll
          for (int i = 0; i < 16; ++i) delta += p[sub][i] * dp[sub][i];
        }
        delta += __shfl_xor(delta, 32);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            p[sub][i] *= dp[sub][i] - delta;  // dSᵀ
            dsum[qt][sub][i] += p[sub][i];
          }
        // the raw scores again (into dP's registers; the operand is made opaque so that the
        // first product's result is not kept alive instead)
        bf16x8 q0 = qf[qt][0], q1 = qf[qt][1];
        asm volatile("" : "+v"(q0), "+v"(q1));
        float ai = 0.f;
        f32x16 dq = zero16();
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
          dp[sub] = mfma32(kf[sub][1], q1, mfma32(kf[sub][0], q0, zero16()));
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            p[sub][i] *= rkL[32 * sub + acc_row(i, hl)];  // dSᵀ·rk_j: G without the lane's rq·τ
            ai += p[sub][i] * dp[sub][i];
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            dq = mfma32(ld_tr(kimg, 32 * sub + 16 * ks, lane), pack_acc(p[sub], ks), dq);
        }
        ai = (ai + __shfl_xor(ai, 32)) * rqt;  // a_i = Σ_j dS_ij·τc_ij
        lsum += ai;
        st_cols_proj(a.dqkv + g.row[qt] * ld + h * D, dq, rqt, qimg + qn * kPitch,
                     proj_factor(rq[qt]) * ai, hl);
        if (hl == 0) {
          stat[qn] = mu;
          stat[64 + qn] = inv_l;
          stat[128 + qn] = delta;
        }
      }
      wave_lds_fence();  // the statistics are written
      // ---- phase B: lane = key
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        __builtin_amdgcn_sched_barrier(0);
        const int kn = 32 * kt + r;
        const uint32_t mb = (g.lasty ? my[kt] : 0u) | (g.lastx ? mx[kt] : 0u);
        const float rkt = rk[kt] * tau;
        float bj = 0.f;
        f32x16 dv = zero16(), dk = zero16();
#pragma unroll
        for (int qs = 0; qs < 2; ++qs) {
          __builtin_amdgcn_sched_barrier(0);
          f32x16 p = mfma32(qf[qs][1], kf[kt][1], mfma32(qf[qs][0], kf[kt][0], zero16()));
          f32x16 ds = mfma32(df[qs][1], vf[kt][1], mfma32(df[qs][0], vf[kt][0], zero16()));
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int qn = 32 * qs + acc_row(i, hl);
            const float rqi = stat[192 + qn];
            const float tc = p[i] * rkt * rqi;  // τc_ij
            float v = tc * kLog2e + E[qn * kEP + kn];
            v += (mb >> (16 * qs + i)) & 1u ? kMaskLog2 : 0.f;
            p[i] = exp2f(v - stat[qn]) * stat[64 + qn];
            const float d = p[i] * (ds[i] - stat[128 + qn]);
            bj += d * tc;
            ds[i] = d * rqi;  // dS·rq_i: G without the lane's rk·τ
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            dv = mfma32(ld_tr(dimg, 32 * qs + 16 * ks, lane), pack_acc(p, ks), dv);
            dk = mfma32(ld_tr(qimg, 32 * qs + 16 * ks, lane), pack_acc(ds, ks), dk);
          }
        }
        bj += __shfl_xor(bj, 32);  // b_j = Σ_i dS_ij·τc_ij
        __bf16* dst = a.dqkv + g.row[kt] * ld + ldo + h * D;
        st_cols_proj(dst, dk, rkt, kimg + kn * kPitch, proj_factor(rk[kt]) * bj, hl);
        st_cols(dst + ldo, dv, 1.f, hl);
      }
    }
  // ---- bias gradient
  dsum_to_E<WS>(E, dsum, wave, lane);
  // ---- logit_scale gradient: both half-waves hold the same a_i, so one half's 32 lanes in a
  // fixed butterfly, then the waves in wave order
  float ls = hl == 0 ? lsum : 0.f;
#pragma unroll
  for (int off = 16; off >= 1; off >>= 1) ls += __shfl_xor(ls, off);
  if (lane == 0) red[wave] = ls;
  __syncthreads();
  if (tid < NREL) {
    st_bias_partial<WS>(E, a, run, h, tid);
  } else if (tid == NREL) {
    float acc = red[0];
#pragma unroll
    for (int wv = 1; wv < kWinWaves; ++wv) acc += red[wv];
    a.partial_ls[(long)run * a.H + h] = a.logit_scale[h] > kLn100 ? 0.f : acc;
  }
}

}  // namespace winattn8

static winattn8::Args winattn8_args(const void* qkv, const float* bias, const float* logit_scale,
                                    int B, int Hs, int Ws, int H, int sy, int sx) {
  winattn8::Args a{};
  wintile::win_geometry<winattn8::WS>(a, qkv, bias, B, Hs, Ws, H, sy, sx);
  a.logit_scale = logit_scale;
  return a;
}

void winattn8_fwd(const void* qkv, const float* bias, const float* logit_scale, void* o, int B,
                  int Hs, int Ws, int H, int sy, int sx, hipStream_t st) {
  winattn8::Args a = winattn8_args(qkv, bias, logit_scale, B, Hs, Ws, H, sy, sx);
  a.o = (__bf16*)o;
  hipLaunchKernelGGL(winattn8::winattn8_fwd_kernel, dim3(a.nruns * H), dim3(64 * kWinWaves), 0,
                     st, a);
}

void winattn8_bwd(const void* dout, const void* qkv, const float* bias, const float* logit_scale,
                  void* dqkv, float* partial, float* dbias, float* dlogit_scale, int B, int Hs,
                  int Ws, int H, int sy, int sx, hipStream_t st) {
  winattn8::Args a = winattn8_args(qkv, bias, logit_scale, B, Hs, Ws, H, sy, sx);
  a.dout = (const __bf16*)dout;
  a.dqkv = (__bf16*)dqkv;
  a.partial = partial;
  a.partial_ls = partial + (long)a.nruns * winattn8::NREL * H;
  hipLaunchKernelGGL(winattn8::winattn8_bwd_kernel, dim3(a.nruns * H), dim3(64 * kWinWaves), 0,
                     st, a);
  det_sum_rows(a.partial, nullptr, a.nruns, winattn8::NREL * H, dbias, nullptr, true, st);
  det_sum_rows(a.partial_ls, nullptr, a.nruns, H, dlogit_scale, nullptr, true, st);
}

}  // namespace mipipe
