// Inference convolution forward: the implicit GEMM of conv_fwd.hip (same tile configs, operand
// paths and split-K plans) with the whole eval-mode tail of a conv block in its epilogue:
//
//   out[m][c] = act( acc[m][c] * scale[c] + shift[c] + residual[m][c] )
//
// scale / shift are a folded eval BatchNorm (bn.hip bn_fold_affine), residual the block input or
// the downsample branch's output, act none or ReLU.  The arithmetic is fp32 on the fp32
// accumulator and the value is rounded once, at the store.  No BN statistics and no tap-flipped
// weight blocks ride in these launches; the training kernels and their EpiParams are untouched.
#include "conv_common.hpp"

namespace mipipe {
using namespace gk;
namespace gk {

struct InferParams {
  void* out;  // bf16 or fp32 [M][N], pitch ldc
  long ldc;
  uint32_t M, N;
  const float* scale;    // per column, null = 1
  const float* shift;    // per column, null = 0
  const void* residual;  // output dtype, [M][ldc], null = none; never aliases out
  int act;               // 0 none, 1 relu
  int nt;                // non-temporal stores of the output tile
};

// The fp32 tile is staged through LDS in PASSES row groups so that one group fits the budget (the
// forward's LDS per block at its promised occupancy): pass p holds accumulator row tiles
// [p*MT/PASSES, (p+1)*MT/PASSES) of every wave row, packed.
template <int BM, int BN, int MT>
constexpr int infer_passes(int budget) {
  int p = 1;
  while (p < MT && (BM / p) * (BN * 4 + 16) > budget) p *= 2;
  return p;
}
template <class T, class C>
constexpr int infer_lds_budget() {
  constexpr int a = main_lds_bytes<T, C>();
  constexpr int b = 160 * 1024 / conv_occ<T, C>();
  return a > b ? a : b;
}
template <class T, class C>
constexpr int infer_passes_for() {
  return infer_passes<C::BM, C::BN, C::BM / C::WM / 16>(infer_lds_budget<T, C>());
}
template <class T, class C>
constexpr int infer_stage_bytes() {
  return (C::BM / infer_passes_for<T, C>()) * (C::BN * 4 + 16);
}

__device__ __forceinline__ void store_nt(uint4* dst, const uint4 v, bool nt) {
  if (nt) __builtin_nontemporal_store(u32v4{v.x, v.y, v.z, v.w}, reinterpret_cast<u32v4*>(dst));
  else *dst = v;
}
__device__ __forceinline__ void store8_nt(__bf16* p, const float* f, bool nt) {
  store_nt(reinterpret_cast<uint4*>(p), pack8(f), nt);
}
__device__ __forceinline__ void store8_nt(float* p, const float* f, bool nt) {
  store_nt(reinterpret_cast<uint4*>(p), make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]),
                                                   __float_as_uint(f[2]), __float_as_uint(f[3])), nt);
  store_nt(reinterpret_cast<uint4*>(p) + 1, make_uint4(__float_as_uint(f[4]), __float_as_uint(f[5]),
                                                       __float_as_uint(f[6]), __float_as_uint(f[7])), nt);
}

// acc layout as epilogue_out: lane holds C[m][n..n+3] of tile (i, j).  A thread of the store
// loop always owns the same 8-column chunk, so its scale / shift are two 8-float vectors loaded
// once, unconditionally at a clamped column (the host checks N % 8 == 0 and 16-B alignment).
// The residual is a ring of 16-B chunks PF iterations ahead, primed after the first pass's
// accumulators went to LDS and issued unconditionally (an absent residual reads the zero line).
template <int BM, int BN, class T, int WM, int WN, bool HALVES, int PASSES>
__device__ void epilogue_infer(char* smem, f32x4 (&acc)[BM / WM / 16][BN / WN / 16],
                               const InferParams& e, uint32_t m0, uint32_t n0, int wave, int lane) {
  constexpr int MT = BM / WM / 16, NT = BN / WN / 16;
  constexpr int kThreads = 64 * WM * WN;
  constexpr int IPP = MT / PASSES;  // accumulator row tiles of a wave per pass
  constexpr int RP = BM / PASSES;   // rows staged per pass
  constexpr int P = BN * 4 + 16;    // fp32 row + 16 B pad
  constexpr int CPR = BN / 8;       // 8-element chunks per row
  constexpr int ITER = RP * CPR / kThreads;
  constexpr int TOTAL = PASSES * ITER;
  constexpr int PF = TOTAL < 4 ? TOTAL : 4;
  static_assert(MT % PASSES == 0 && kThreads % CPR == 0 && (RP * CPR) % kThreads == 0,
                "inference epilogue thread map");
  typedef AccMap<BM, BN, WM, WN, HALVES> Map;
  const int wr = wave / WN, wc = wave % WN;
  const uint32_t lr = lane & 15, lc = (lane >> 4) * 4;
  const uint32_t my_cc = threadIdx.x % CPR, my_n = n0 + my_cc * 8;
  const uint32_t ld_n = my_n < e.N ? my_n : 0;
  const bool has_res = e.residual != nullptr;
  const float* zf = reinterpret_cast<const float*>(g_epi_zero);
  float sc[8], sh[8];
  ld_f32x8(e.scale != nullptr ? e.scale + ld_n : zf, sc);
  ld_f32x8(e.shift != nullptr ? e.shift + ld_n : zf, sh);
  if (e.scale == nullptr) {
#pragma unroll
    for (int q = 0; q < 8; ++q) sc[q] = 1.f;
  }
  if (e.shift == nullptr) {  // -0: v*1 + (-0) is v for every v, -0 included
#pragma unroll
    for (int q = 0; q < 8; ++q) sh[q] = -0.f;
  }
  // tile-local output row of this thread's chunk in (pass-major) iteration g
  auto tile_row = [&](int g) -> uint32_t {
    const uint32_t r = (threadIdx.x + (g % ITER) * kThreads) / CPR;
    const uint32_t blk = r >> 4;
    return Map::row((int)(blk / IPP), (g / ITER) * IPP + (int)(blk % IPP)) + (r & 15);
  };
  const T* rp = has_res ? reinterpret_cast<const T*>(e.residual) : reinterpret_cast<const T*>(g_epi_zero);
  Raw8<T> ring[PF];
  auto issue = [&](int g, int slot) {
    const uint32_t m = min(m0 + tile_row(g), e.M - 1);
    ring[slot] = ld_raw8(rp + (has_res ? (long)m * e.ldc + ld_n : 0));
  };
  T* C = reinterpret_cast<T*>(e.out);
  // the activation is a wave-uniform branch around the whole loop, not a per-element select
  auto run = [&](auto relu_tag) {
    constexpr bool RELU = decltype(relu_tag)::value;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      // every wave is past the main loop (p == 0) / the previous pass's staging reads
      lds_barrier();
#pragma unroll
      for (int ii = 0; ii < IPP; ++ii)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int i = p * IPP + ii;
          const uint32_t ml = (uint32_t)(wr * IPP + ii) * 16 + lr, nl = Map::col(wc, j) + lc;
          *reinterpret_cast<float4*>(smem + ml * P + nl * 4) =
              make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
      if (p == 0) {
#pragma unroll
        for (int k = 0; k < PF; ++k) issue(k, k);
      }
      lds_barrier();
#pragma unroll
      for (int it = 0; it < ITER; ++it) {
        const int g = p * ITER + it;
        const uint32_t r = (threadIdx.x + it * kThreads) / CPR;
        const float4 lo = *reinterpret_cast<const float4*>(smem + r * P + my_cc * 32);
        const float4 hi = *reinterpret_cast<const float4*>(smem + r * P + my_cc * 32 + 16);
        float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}, a[8];
        unpack_raw(ring[g % PF], a);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          float v = fmaf(f[q], sc[q], sh[q]);
          v = has_res ? v + a[q] : v;
          f[q] = RELU ? fmaxf(v, 0.f) : v;
        }
        const uint32_t m = m0 + tile_row(g);
        if (m < e.M && my_n < e.N) store8_nt(C + (long)m * e.ldc + my_n, f, e.nt != 0);
        if (g + PF < TOTAL) issue(g + PF, g % PF);
      }
    }
  };
  if (e.act == 1) run(std::true_type());
  else run(std::false_type());
}

template <class T, class C>
constexpr int conv_infer_lds_bytes() {
  return main_lds_bytes<T, C>() > infer_stage_bytes<T, C>() ? main_lds_bytes<T, C>()
                                                             : infer_stage_bytes<T, C>();
}

// conv_fwd_kernel's main loop (conv_common.hpp) with the inference epilogue.
template <class C, bool DENSE, bool ALIGNED, class T>
__global__ __launch_bounds__(C::THREADS, (conv_occ<T, C>())) void conv_infer_kernel(
    const T* __restrict__ x, const T* __restrict__ w, ConvGeom g, uint32_t M, uint32_t tilesN,
    InferParams e) {
  constexpr int BM = C::BM, BN = C::BN;
  typedef typename std::conditional<DENSE, PolKCDense<T>, PolKCIm2col<ALIGNED, T>>::type PA;
  __shared__ __attribute__((aligned(16))) char smem[conv_infer_lds_bytes<T, C>()];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const uint32_t id = xcd_remap(blockIdx.x, gridDim.x);
  const uint32_t tm = id / tilesN, tn = id % tilesN;
  const uint32_t m0 = tm * BM, n0 = tn * BN;
  const uint32_t K = (uint32_t)(g.KH * g.KW * g.C);
  const int nk = (int)((K + BK - 1) / BK);
  auto ia = [&](auto& a, uint32_t origin) {
    if constexpr (DENSE) a.init(x, g.C, M, K, origin, wave, lane, g_conv_zero);
    else a.init(x, g, M, origin, wave, lane, g_conv_zero);
  };
  auto ib = [&](auto& b, uint32_t origin) { b.init(w, K, e.N, K, origin, wave, lane, g_conv_zero); };
  f32x4 acc[BM / C::WM / 16][BN / C::WN / 16];
  run_main_loop<T, C, PA, PolKCDense<T>>(smem, ia, ib, m0, n0, 0, nk, acc, wave, lane);
  epilogue_infer<BM, BN, T, C::WM, C::WN, C::PP, infer_passes_for<T, C>()>(smem, acc, e, m0, n0,
                                                                            wave, lane);
}

// Finish of a split-K plan (the partial tiles come from conv_fwd.hip's split launch): the
// slices are summed per accumulator position in slice order, as conv_splitk_finish_kernel does,
// then the inference epilogue runs on the sum.
template <class C, class T>
__global__ __launch_bounds__(C::THREADS) void conv_infer_finish_kernel(
    const float* __restrict__ ws, int S, uint32_t tilesN, InferParams e) {
  constexpr int BM = C::BM, BN = C::BN, WM = C::WM, WN = C::WN;
  constexpr int MT = BM / WM / 16, NT = BN / WN / 16;
  __shared__ __attribute__((aligned(16))) char smem[infer_stage_bytes<T, C>()];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const uint32_t tm = blockIdx.x / tilesN, tn = blockIdx.x % tilesN;
  const uint32_t m0 = tm * BM, n0 = tn * BN;
  const int wr = wave / WN, wc = wave % WN;
  typedef AccMap<BM, BN, WM, WN, false> Map;
  const uint32_t lr = lane & 15, lc = (lane >> 4) * 4;
  const long slice = (long)e.M * e.N;
  // element offsets of this lane's rows / column quads (clamped: masked at the store); kept as
  // MT + NT values, not MT * NT, so the 256x256 tile's 128 accumulators leave room for them
  // (the host checks M * N < 2^31)
  uint32_t roff[MT], coff[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) roff[i] = min(m0 + Map::row(wr, i) + lr, e.M - 1) * e.N;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const uint32_t n = n0 + Map::col(wc, j) + lc;
    coff[j] = n < e.N ? n : 0;
  }
  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(ws + roff[i] + coff[j]);
      acc[i][j] = f32x4{v.x, v.y, v.z, v.w};
    }
  for (int s = 1; s < S; ++s) {  // slice order: deterministic
    const float* wsl = ws + s * slice;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(wsl + roff[i] + coff[j]);
        acc[i][j] += f32x4{v.x, v.y, v.z, v.w};
        // the 128-accumulator tiles: at most half a slice's loads in flight beside the
        // accumulators (all of them at once spilled the 8-wave 256x256 tile to scratch)
        if (MT * NT >= 32 && i == MT / 2 - 1 && j == NT - 1) __builtin_amdgcn_sched_barrier(0);
      }
  }
  epilogue_infer<BM, BN, T, WM, WN, false, infer_passes_for<T, C>()>(smem, acc, e, m0, n0, wave,
                                                                     lane);
}

}  // namespace gk

template <class T>
static void conv_fwd_infer_t(const void* x, const void* w, void* y, const ConvShape& s,
                             hipStream_t st, const float* scale, const float* shift,
                             const void* residual, bool relu, int cfg, float* split_ws) {
  ConvGeom g = make_geom(s);
  const uint32_t M = (uint32_t)s.N * s.Ho * s.Wo;
  InferParams e{};
  e.out = y; e.ldc = s.Co; e.M = M; e.N = s.Co;
  e.scale = scale; e.shift = shift; e.residual = residual; e.act = relu ? 1 : 0;
  e.nt = (g_nt_store & 1) && (long)M * s.Co * (s.f32 ? 4 : 2) > g_nt_min_bytes;
  // a split-K plan: conv_fwd.hip's partial-tile launch, then the finish kernel of this file
  int S = 1;
  if (split_ws != nullptr) S = conv_fwd_split_partials(x, w, s, st, cfg, split_ws);
  cfg = resolve_fwd_cfg(s, cfg);
  const bool dense = is_dense(s);
  const bool aligned = s.Ci % BK == 0 && (s.f32 || s.KH * s.KW <= 32);  // as conv_fwd
  const T* xp = (const T*)x;
  const T* wp = (const T*)w;
  with_tile<T>(cfg, [&](auto tile) {
    typedef decltype(tile) C;
    const uint32_t tN = cdiv(s.Co, C::BN), tiles = cdiv(M, C::BM) * tN;
    const dim3 block(C::THREADS);
    if (S > 1) {
      hipLaunchKernelGGL((conv_infer_finish_kernel<C, T>), dim3(tiles), block, 0, st,
                         (const float*)split_ws, S, tN, e);
      return;
    }
    const dim3 grid(tiles);
    if (dense)
      hipLaunchKernelGGL((conv_infer_kernel<C, true, false, T>), grid, block, 0, st, xp, wp, g, M, tN, e);
    else if (aligned)
      hipLaunchKernelGGL((conv_infer_kernel<C, false, true, T>), grid, block, 0, st, xp, wp, g, M, tN, e);
    else
      hipLaunchKernelGGL((conv_infer_kernel<C, false, false, T>), grid, block, 0, st, xp, wp, g, M, tN, e);
  });
}

void conv_fwd_infer(const void* x, const void* w, void* y, const ConvShape& s, hipStream_t st,
                    const float* scale, const float* shift, const void* residual, bool relu,
                    int cfg, float* split_ws) {
  if (s.f32) conv_fwd_infer_t<float>(x, w, y, s, st, scale, shift, residual, relu, cfg, split_ws);
  else conv_fwd_infer_t<__bf16>(x, w, y, s, st, scale, shift, residual, relu, cfg, split_ws);
}

}  // namespace mipipe
