// Evaluation statistics of one batch of logits [R, V] in one launch (mipipe/metrics.py): top-1 and
// top-k hits, the cross-entropy sum, a confidence histogram (for ECE and the confidence curve) and
// the confusion matrix, all from the one read of the row that top1_correct already does.  The
// results accumulate in device buffers; no host value is read back per batch.
//
// Per row r with label y (Vv = valid_cols when 0 < valid_cols < V, else V; columns >= Vv pad the
// vocabulary and enter no result):
//   y == ignore_index        the row is skipped, counted nowhere
//   y < 0 or y >= Vv         counters[invalid] += 1, nothing is read or written through y
//   order on logits          top1_correct's: NaN is greater than every number, NaNs are equal
//   pred                     the first maximal index (torch.argmax's tie rule); a row of nothing
//                            but -inf predicts column 0, where top1_correct finds no maximum
//                            and never counts a hit (the one input on which the two differ)
//   rank                     #{c < Vv : x[c] > x[y]} + #{c < y : x[c] == x[y]}
//                            top-1 hit: pred == y (rank == 0); top-k hit: rank < k
//   loss                     lse - x[y] in fp32, lse from an online log-sum-exp (running max)
//   conf                     exp(max - lse), bin = min(bins - 1, floor(conf * bins))
// x[y] is loaded first; max / argmax, the two rank counts and the log-sum-exp then come from one
// pass over the row.  A row whose loss is not finite or exceeds 2^16 goes to counters[nonfinite]
// and stays out of the loss sum and the histogram; its top-k and confusion entries still count.
//
// Sums are integers.  The loss (clamped at 0) and the confidence are rounded to nearest into Q24
// fixed point and added with integer atomics, so every buffer is independent of the order of the
// adds: bit-identical from run to run and for any split of the rows over batches or ranks (a float
// atomic or a second launch would not give that).  Capacity of the int64 loss sum: a row adds at
// most 2^16 * 2^24 = 2^40, so 2^23 rows cannot overflow it unless every one of them sits exactly
// at the 2^16 cap (2^23 - 1 such rows still fit); a confidence adds at most 2^24 (+1 ulp).
//
//   counters  int64 [8]        rows, top1, topk, nonfinite, invalid, loss_q24, 0, 0
//   hist      int64 [3, bins]  wrong predictions, correct predictions, Q24 sum of conf; may be null
//   cm        int32 [Vv, Vv]   cm[y, pred] += 1; may be null (a 30,528-column vocabulary)
//
// Shape: top1_correct's one wave per row, four rows per block.  Rows are read with 16-byte loads
// when every row start is 16-byte aligned (V * sizeof(T) % 16 == 0 and an aligned base), with
// scalar loads otherwise.  The counters are summed over the block's four rows in LDS and leave
// with one atomic per non-zero counter per block; histogram and confusion adds go to global
// memory directly (they spread over many addresses).  No float atomics anywhere.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   eval_stats_kernel<float,  true>   VGPRs 25, SGPRs 49, scratch 0, LDS 192 B, 8 waves/SIMD
//   eval_stats_kernel<float,  false>  VGPRs 25, SGPRs 41, scratch 0, LDS 192 B, 8 waves/SIMD
//   eval_stats_kernel<__bf16, true>   VGPRs 25, SGPRs 49, scratch 0, LDS 192 B, 8 waves/SIMD
//   eval_stats_kernel<__bf16, false>  VGPRs 25, SGPRs 41, scratch 0, LDS 192 B, 8 waves/SIMD
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

namespace {

constexpr int kEvalCounters = 6;  // rows, top1, topk, nonfinite, invalid, loss_q24
constexpr float kQ24 = 16777216.f;
constexpr float kLossCap = 65536.f;

// the total order of top1_correct: NaN above every number, NaNs equal to each other
__device__ __forceinline__ bool ord_gt(float a, float b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ bool ord_eq(float a, float b) { return a == b || (a != a && b != b); }

// Per-lane (later per-wave) state of the single pass over a row.
struct RowState {
  float best;  // maximum under the total order
  int arg;     // its first index; 0x7fffffff: no column seen yet
  int gt, eq;  // the two rank counts
  float m, s;  // online log-sum-exp: running max and sum of exp(x - m)
};

__device__ __forceinline__ void row_step(RowState& st, float v, int c, float xy, int y) {
  if (st.arg == 0x7fffffff || ord_gt(v, st.best)) {  // strictly greater keeps the first index
    st.best = v;
    st.arg = c;
  }
  st.gt += ord_gt(v, xy) ? 1 : 0;
  st.eq += (c < y && ord_eq(v, xy)) ? 1 : 0;
  // v == m covers (-inf) - (-inf) and inf - inf; a NaN makes s NaN
  if (v > st.m) {
    st.s = st.s * expf(st.m - v) + 1.f;
    st.m = v;
  } else {
    st.s += v == st.m ? 1.f : expf(v - st.m);
  }
}

template <class T, bool VEC>
__global__ __launch_bounds__(256) void eval_stats_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ labels, int R, int V, int Vv, int k,
    int64_t ignore_index, int bins, unsigned long long* __restrict__ counters,
    unsigned long long* __restrict__ hist, int* __restrict__ cm) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  __shared__ unsigned long long part[4][kEvalCounters];
  if (lane < kEvalCounters) part[wave][lane] = 0;
  if (row < R) {
    const int64_t y64 = labels[row];
    const bool valid = y64 != ignore_index && y64 >= 0 && y64 < (int64_t)Vv;
    if (!valid) {
      if (lane == 0 && y64 != ignore_index) part[wave][4] = 1;
    } else {
      const int y = (int)y64;
      const T* x = logits + (long)row * V;
      const float xy = to_f32(x[y]);
      RowState st{-INFINITY, 0x7fffffff, 0, 0, -INFINITY, 0.f};
      if constexpr (VEC) {
        constexpr int E = 16 / (int)sizeof(T);  // elements per 16-byte load
        // V % E == 0: a chunk that starts below Vv <= V ends inside the row
        for (int c0 = lane * E; c0 < Vv; c0 += 64 * E) {
          float f[E];
          if constexpr (E == 8) {
            unpack8(*reinterpret_cast<const uint4*>(x + c0), f);
          } else {
            const float4 a = *reinterpret_cast<const float4*>(x + c0);
            f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
          }
#pragma unroll
          for (int j = 0; j < E; ++j)
            if (c0 + j < Vv) row_step(st, f[j], c0 + j, xy, y);
        }
      } else {
        for (int c = lane; c < Vv; c += 64) row_step(st, to_f32(x[c]), c, xy, y);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(st.best, o);
        const int oa = __shfl_xor(st.arg, o);
        // a lane that saw no column has arg 0x7fffffff and loses every comparison
        if (oa != 0x7fffffff &&
            (st.arg == 0x7fffffff || ord_gt(ob, st.best) || (ord_eq(ob, st.best) && oa < st.arg))) {
          st.best = ob;
          st.arg = oa;
        }
        st.gt += __shfl_xor(st.gt, o);
        st.eq += __shfl_xor(st.eq, o);
        const float om = __shfl_xor(st.m, o);
        const float os = __shfl_xor(st.s, o);
        const float nm = fmaxf(st.m, om);  // neither is NaN: a NaN only ever enters s
        st.s = st.s * (st.m == nm ? 1.f : expf(st.m - nm)) + os * (om == nm ? 1.f : expf(om - nm));
        st.m = nm;
      }
      if (lane == 0) {
        const int pred = st.arg;  // Vv >= 1: lane 0 saw column 0, so pred < Vv
        const bool hit = pred == y;
        const float lse = st.m + logf(st.s);
        const float loss = lse - xy;
        const bool finite = loss == loss && fabsf(loss) != INFINITY && loss <= kLossCap;
        part[wave][0] = 1;
        part[wave][1] = hit ? 1 : 0;
        part[wave][2] = st.gt + st.eq < k ? 1 : 0;
        part[wave][3] = finite ? 0 : 1;
        if (finite) {
          part[wave][5] = (unsigned long long)llrintf(fmaxf(loss, 0.f) * kQ24);
          if (hist != nullptr) {
            const float conf = expf(st.best - lse);
            const int bin = min(bins - 1, max(0, (int)floorf(conf * (float)bins)));
            atomicAdd(hist + (hit ? bins : 0) + bin, 1ull);
            atomicAdd(hist + 2 * bins + bin, (unsigned long long)llrintf(conf * kQ24));
          }
        }
        if (cm != nullptr && (unsigned)pred < (unsigned)Vv) atomicAdd(cm + (long)y * Vv + pred, 1);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kEvalCounters) {
    const int i = threadIdx.x;
    const unsigned long long v = part[0][i] + part[1][i] + part[2][i] + part[3][i];
    if (v) atomicAdd(counters + i, v);
  }
}

}  // namespace

void eval_stats(const void* logits, const int64_t* labels, int R, int V, int Vv, int k,
                int64_t ignore_index, int bins, int64_t* counters, int64_t* hist, int* cm,
                hipStream_t st, bool f32) {
  if (R <= 0) return;
  if (Vv <= 0 || Vv > V) Vv = V;
  const dim3 g((unsigned)(((long)R + 3) / 4));
  const size_t esz = f32 ? 4 : 2;
  const bool vec = ((size_t)V * esz) % 16 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  auto go = [&](auto t, auto vec_c) {
    using T = decltype(t);
    hipLaunchKernelGGL((eval_stats_kernel<T, decltype(vec_c)::value>), g, dim3(256), 0, st,
                       (const T*)logits, labels, R, V, Vv, k, ignore_index, bins,
                       reinterpret_cast<unsigned long long*>(counters),
                       reinterpret_cast<unsigned long long*>(hist), cm);
  };
  if (f32) {
    if (vec) go(float(), std::true_type());
    else go(float(), std::false_type());
  } else {
    if (vec) go(__bf16(), std::true_type());
    else go(__bf16(), std::false_type());
  }
}

}  // namespace mipipe
