// Batch mixing for the training step: Mixup and CutMix of an NCHW batch with its own reverse
// (sample i is paired with sample B-1-i, timm's flip(0) pairing), in place or into a second
// tensor.  What to do is read from a device-side fp32[8] descriptor (mipipe/data/mix.py):
//   [0] lambda, [1] mode (0 none, 1 mixup, 2 cutmix), [2..5] y0, y1, x0, x1 of the box.
// No host value enters the launch: grid and arguments depend on the shape alone, so a captured
// hipGraph replays with whatever the descriptor holds at that step.
//
//   mode 0: out = x (in place: nothing is read or written)
//   mode 1: out[i] = lambda * x[i] + (1 - lambda) * x[B-1-i]: two rounded fp32 multiplies and one
//           rounded add (contraction off, as in records.hip), 1 - lambda an fp32 subtraction,
//           the sum rounded once to the output type
//   mode 2: out[i] = x[B-1-i] inside the box, x[i] outside
//
// A streaming pass.  One work unit owns a slice of a PAIR (i, B-1-i): each element of the two
// samples is read once and both results are written by the same lane, so the in-place form has
// no hazard and moves 2 reads + 2 writes per two elements.  The self-paired middle sample of an
// odd batch is handled once and keeps its bits in every mode (lambda * a + (1 - lambda) * a is a;
// the rounded sum would only be near it): copied out of place, untouched in place.  In-place
// CutMix swaps only the box: rows y0..y1 of every channel, columns x0..x1, traffic proportional
// to the box area.  Everything else runs over the sample as
// one contiguous run of C*H*W elements (the out-of-place CutMix decides per element whether it
// lies in the box).  A run is a scalar head up to the first 16-byte boundary, 16-byte accesses
// per lane, and a scalar tail; a pair whose four rows do not share one alignment (C*H*W * size
// not a multiple of 16) goes element by element.
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

constexpr int kMixThreads = 256;
constexpr int kMixMaxBlocks = 2048;

template <class T>
struct MixBits;
template <>
struct MixBits<float> {
  using U = uint32_t;
  static __device__ __forceinline__ float get(U b) { return __uint_as_float(b); }
  static __device__ __forceinline__ U put(float f) { return __float_as_uint(f); }
};
template <>
struct MixBits<__bf16> {
  using U = uint16_t;
  static __device__ __forceinline__ float get(U b) { return bf16_bits_to_f(b); }
  static __device__ __forceinline__ U put(float f) {
    const __bf16 v = (__bf16)f;  // round to nearest even
    return __builtin_bit_cast(uint16_t, v);
  }
};

// lam * a + om * b in three roundings (hipcc would contract the add into v_fma_f32)
__device__ __forceinline__ float mix2(float lam, float a, float om, float b) {
#pragma clang fp contract(off)
  const float p = lam * a;
  const float q = om * b;
  return p + q;
}

struct MixOp {
  float lam, om;
  int mode;      // 0 copy, 1 mixup, 2 cutmix
  bool box_run;  // the run lies inside the box: every element is swapped
  int y0, y1, x0, x1;
  FastDiv fW, fH;
  int W, H;
};

// results for the pair's two samples from their elements a, b at flat sample offset e
template <class T>
__device__ __forceinline__ void mix_elem(const MixOp& op, int mode, typename MixBits<T>::U a,
                                         typename MixBits<T>::U b, uint32_t e,
                                         typename MixBits<T>::U& ra, typename MixBits<T>::U& rb) {
  using M = MixBits<T>;
  if (mode == 1) {
    const float fa = M::get(a), fb = M::get(b);
    ra = M::put(mix2(op.lam, fa, op.om, fb));
    rb = M::put(mix2(op.lam, fb, op.om, fa));
    return;
  }
  bool sw = false;
  if (mode == 2) {
    sw = op.box_run;
    if (!sw) {
      const uint32_t row = op.fW.div(e);  // c * H + y
      const int xx = (int)(e - row * (uint32_t)op.W);
      const int y = (int)(row - op.fH.div(row) * (uint32_t)op.H);
      sw = y >= op.y0 && y < op.y1 && xx >= op.x0 && xx < op.x1;
    }
  }
  ra = sw ? b : a;
  rb = sw ? a : b;
}

// x and out may be the same tensor: no __restrict__ on them
template <class T>
__global__ __launch_bounds__(kMixThreads) void batch_mix_kernel(
    const T* x, T* out, const float* __restrict__ mix, int B, int C, int H, int W, int slices,
    FastDiv fW, FastDiv fH) {
  using M = MixBits<T>;
  using U = typename M::U;
  constexpr int V = 16 / (int)sizeof(T);
  const bool inplace = (const T*)out == x;
  MixOp op;
  op.lam = mix[0];
  op.om = 1.f - op.lam;
  const int m = (int)mix[1];
  op.mode = (m == 1 || m == 2) ? m : 0;
  // the box, clamped into the image whatever the descriptor holds
  op.y0 = min(max((int)mix[2], 0), H);
  op.y1 = min(max((int)mix[3], op.y0), H);
  op.x0 = min(max((int)mix[4], 0), W);
  op.x1 = min(max((int)mix[5], op.x0), W);
  op.fW = fW;
  op.fH = fH;
  op.W = W;
  op.H = H;
  op.box_run = op.mode == 2 && inplace;
  if (op.mode == 0 && inplace) return;
  const uint32_t per = (uint32_t)C * H * W;
  const int bh = op.y1 - op.y0, bw = op.x1 - op.x0;
  if (op.box_run && (bh <= 0 || bw <= 0)) return;
  // runs of one sample: the box's rows (in-place cutmix) or the whole sample
  const uint32_t nrows = op.box_run ? (uint32_t)C * bh : 1u;
  const uint32_t L = op.box_run ? (uint32_t)bw : per;
  const int npairs = (B + 1) / 2;
  const long units = (long)npairs * slices;
  const U* xu = reinterpret_cast<const U*>(x);
  U* ou = reinterpret_cast<U*>(out);
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const int i = (int)(u / slices);
    const int slice = (int)(u - (long)i * slices);
    const int j = B - 1 - i;
    const bool self = i == j;
    if (self && inplace) continue;   // a sample mixed with itself is itself
    const int mode = self ? 0 : op.mode;  // out of place: copied
    const U* sa = xu + (long)i * per;
    const U* sb = xu + (long)j * per;
    U* da = ou + (long)i * per;
    U* db = ou + (long)j * per;
    // one alignment for the four rows of every run <=> the sample bases agree mod 16 bytes
    const uint32_t ma = (uint32_t)(reinterpret_cast<uintptr_t>(sa) & 15);
    const bool co = ma == (uint32_t)(reinterpret_cast<uintptr_t>(sb) & 15) &&
                    ma == (uint32_t)(reinterpret_cast<uintptr_t>(da) & 15) &&
                    ma == (uint32_t)(reinterpret_cast<uintptr_t>(db) & 15);
    // items of a run: [head | 16-byte vectors | tail], or single elements
    const uint32_t ipr = co ? L / V + 2 : L;
    const unsigned long items = (unsigned long)nrows * ipr;
    for (unsigned long it = (unsigned long)slice * kMixThreads + threadIdx.x; it < items;
         it += (unsigned long)slices * kMixThreads) {
      const uint32_t row = (uint32_t)it / ipr;  // items < 2^32: nrows * (L + 2) <= per + 2 C H
      const uint32_t k = (uint32_t)it - row * ipr;
      uint32_t off = 0;
      if (op.box_run) {
        const uint32_t c = row / (uint32_t)bh;
        const uint32_t y = (uint32_t)op.y0 + row - c * (uint32_t)bh;
        off = (c * (uint32_t)H + y) * (uint32_t)W + (uint32_t)op.x0;
      }
      if (!co) {
        const uint32_t e = off + k;
        U ra, rb;
        mix_elem<T>(op, mode, sa[e], sb[e], e, ra, rb);
        da[e] = ra;
        if (!self) db[e] = rb;
        continue;
      }
      // elements until the first 16-byte boundary of this run
      const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(sa + off) & 15) / sizeof(T));
      const uint32_t head = min(L, (V - mis) % V);
      const uint32_t nvec = (L - head) / V;
      if (k >= 1 && k <= nvec) {
        const uint32_t e0 = off + head + (k - 1) * V;
        const uint4 qa = *reinterpret_cast<const uint4*>(sa + e0);
        const uint4 qb = *reinterpret_cast<const uint4*>(sb + e0);
        U va[V], vb[V], wa[V], wb[V];
        __builtin_memcpy(va, &qa, 16);
        __builtin_memcpy(vb, &qb, 16);
#pragma unroll
        for (int q = 0; q < V; ++q) mix_elem<T>(op, mode, va[q], vb[q], e0 + q, wa[q], wb[q]);
        uint4 oa, ob;
        __builtin_memcpy(&oa, wa, 16);
        __builtin_memcpy(&ob, wb, 16);
        *reinterpret_cast<uint4*>(da + e0) = oa;
        if (!self) *reinterpret_cast<uint4*>(db + e0) = ob;
      } else if (k == 0 || k == nvec + 1) {
        const uint32_t b0 = k == 0 ? 0 : head + nvec * V;
        const uint32_t b1 = k == 0 ? head : L;
        for (uint32_t q = b0; q < b1; ++q) {
          const uint32_t e = off + q;
          U ra, rb;
          mix_elem<T>(op, mode, sa[e], sb[e], e, ra, rb);
          da[e] = ra;
          if (!self) db[e] = rb;
        }
      }
    }
  }
}

}  // namespace

void batch_mix(const void* x, void* out, const float* mix, int B, int C, int H, int W, bool f32,
               hipStream_t st) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return;
  const long per = (long)C * H * W;
  const int V = f32 ? 4 : 8;
  const int npairs = (B + 1) / 2;
  // slices of a pair: enough units to fill the capped grid, at most one per 256 vectors
  const long by_size = std::max<long>(1, (per / V + kMixThreads - 1) / kMixThreads);
  const long by_grid = std::max<long>(1, (2 * kMixMaxBlocks + npairs - 1) / npairs);
  const int slices = (int)std::min(by_size, by_grid);
  const int grid = (int)std::min<long>((long)npairs * slices, kMixMaxBlocks);
  const FastDiv fW((uint32_t)W), fH((uint32_t)H);
  if (f32)
    hipLaunchKernelGGL(batch_mix_kernel<float>, dim3(grid), dim3(kMixThreads), 0, st,
                       (const float*)x, (float*)out, mix, B, C, H, W, slices, fW, fH);
  else
    hipLaunchKernelGGL(batch_mix_kernel<__bf16>, dim3(grid), dim3(kMixThreads), 0, st,
                       (const __bf16*)x, (__bf16*)out, mix, B, C, H, W, slices, fW, fH);
}

}  // namespace mipipe
