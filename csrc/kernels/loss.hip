// The loss of the training step and the top-1 count of the eval loop: cross-entropy in its fused
// form (loss and gradient in one pass over the logits; the tests' cross-check) and its split
// form (forward keeps the row log-sum-exps, backward writes the gradient from the logits), hard
// labels or Mixup / CutMix pair targets.  16-B vector accesses where V % kCeVec == 0.
#include "common.hpp"
#include "launchers.hpp"

namespace mipipe {

// ------------------------------------------------------------------------------ cross-entropy
__global__ void ce_count_kernel(const int64_t* __restrict__ labels, int R, int64_t ignore,
                                int* __restrict__ out) {
  __shared__ int red[kCeThreads];
  int c = 0;
  for (int i = threadIdx.x; i < R; i += kCeThreads) c += labels[i] != ignore;
  red[threadIdx.x] = c;
  __syncthreads();
  for (int s = kCeThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

__device__ __forceinline__ float block_reduce(float v, float* sh, bool is_max) {
  v = is_max ? wave_max(v) : wave_sum(v);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = is_max ? fmaxf(r, sh[i]) : r + sh[i];
  return r;
}

// The logit of a row's label.  A label outside the classes reads nothing (its logit counts as
// 0): hard labels other than ignore_index and both labels of a pair target alike.  The gradient
// needs no such guard: a column's target is used only where col < Vv, and no such column equals a
// label outside [0, Vv).
template <class T>
__device__ __forceinline__ float ce_label_logit(const T* x, int64_t lab, int Vv) {
  return (uint64_t)lab < (uint64_t)Vv ? (float)x[lab] : 0.f;
}

// Loss of one counted row; sx: the sum of the row's class logits.  Without smoothing the
// smoothing term is left out, not multiplied by 0: a masked class (-inf) makes sx -inf, and
// 0 * inf would turn a finite loss into NaN.  (The smoothed expression stays one expression, as
// it always was, so that its contraction into FMAs, and with it every bit for eps > 0, stays.)
__device__ __forceinline__ float ce_row_loss(float lse, float xl, float sx, int Vv, float eps) {
  const float smoothed = (1.f - eps) * (lse - xl) + eps * (lse - sx / (float)Vv);
  return eps > 0.f ? smoothed : lse - xl;
}

// one block per row; logits T (bf16 / fp32) [R][V] of which the first Vv columns are classes
// (the rest: tile padding of the vocabulary, excluded from the softmax, gradient 0)
template <class T>
__global__ __launch_bounds__(kCeThreads) void ce_kernel(const T* __restrict__ logits,
                                                 const int64_t* __restrict__ labels,
                                                 float* __restrict__ loss, T* __restrict__ grad,
                                                 int V, int Vv, float eps, int64_t ignore,
                                                 const int* __restrict__ nvalid,
                                                 float* __restrict__ rowloss) {
  __shared__ float sh[kCeThreads / 64];
  const long row = blockIdx.x;
  const T* x = logits + row * V;
  T* g = grad + row * V;
  const int64_t lab = labels[row];
  const bool valid = lab != ignore;
  const bool vec = (V % kCeVec) == 0;
  float mx = -INFINITY, sx = 0.f;
  if (vec) {
    for (int c = threadIdx.x; c < V / kCeVec; c += kCeThreads) {
      float v[kCeVec];
      load8(x + c * kCeVec, v);
#pragma unroll
      for (int q = 0; q < kCeVec; ++q) {
        if (c * kCeVec + q < Vv) {
          mx = fmaxf(mx, v[q]);
          sx += v[q];
        }
      }
    }
  } else {
    for (int c = threadIdx.x; c < Vv; c += kCeThreads) {
      float v = (float)x[c];
      mx = fmaxf(mx, v);
      sx += v;
    }
  }
  mx = block_reduce(mx, sh, true);
  sx = block_reduce(sx, sh, false);
  float se = 0.f;
  if (vec) {
    for (int c = threadIdx.x; c < V / kCeVec; c += kCeThreads) {
      float v[kCeVec];
      load8(x + c * kCeVec, v);
#pragma unroll
      for (int q = 0; q < kCeVec; ++q)
        if (c * kCeVec + q < Vv) se += __expf(v[q] - mx);
    }
  } else {
    for (int c = threadIdx.x; c < Vv; c += kCeThreads) se += __expf((float)x[c] - mx);
  }
  se = block_reduce(se, sh, false);
  const float lse = mx + __logf(se);
  const float inv_n = 1.f / (float)max(1, nvalid[0]);
  if (threadIdx.x == 0) {  // summed in a fixed order by ce_sum_kernel (no float atomics)
    float l = 0.f;
    if (valid) {
      const float xl = ce_label_logit(x, lab, Vv);
      l = ce_row_loss(lse, xl, sx, Vv, eps);
    }
    rowloss[row] = l * inv_n;
  }
  const float scale = valid ? inv_n : 0.f;
  const float inv_se = 1.f / se;
  const float base_t = eps / (float)Vv;
  if (vec) {
    for (int c = threadIdx.x; c < V / kCeVec; c += kCeThreads) {
      float v[kCeVec];
      load8(x + c * kCeVec, v);
#pragma unroll
      for (int q = 0; q < kCeVec; ++q) {
        int col = c * kCeVec + q;
        float t = base_t + (col == lab ? 1.f - eps : 0.f);
        v[q] = col < Vv ? (__expf(v[q] - mx) * inv_se - t) * scale : 0.f;
      }
      store8(g + c * kCeVec, v);
    }
  } else {
    for (int c = threadIdx.x; c < V; c += kCeThreads) {
      float t = base_t + (c == lab ? 1.f - eps : 0.f);
      g[c] = (T)(c < Vv ? (__expf((float)x[c] - mx) * inv_se - t) * scale : 0.f);
    }
  }
}

// loss = sum of the per-row losses in a fixed order (thread t: rows t, t + kCeThreads, ...; then a tree)
__global__ __launch_bounds__(kCeThreads) void ce_sum_kernel(const float* __restrict__ rowloss, int R,
                                                     float* __restrict__ loss) {
  __shared__ float red[kCeThreads];
  float a = 0.f;
  for (int i = threadIdx.x; i < R; i += kCeThreads) a += rowloss[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = kCeThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = red[0];
}

void cross_entropy_fwd_bwd(const void* logits, const int64_t* labels, float* loss, void* grad,
                           int R, int V, float smoothing, int64_t ignore_index, int* work,
                           hipStream_t st, bool f32, int Vv) {
  if (Vv <= 0 || Vv > V) Vv = V;
  float* rowloss = reinterpret_cast<float*>(work + 4);
  hipLaunchKernelGGL(ce_count_kernel, dim3(1), dim3(kCeThreads), 0, st, labels, R, ignore_index, work);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ce_kernel<T>, dim3(R), dim3(kCeThreads), 0, st, (const T*)logits, labels, loss,
                       (T*)grad, V, Vv, smoothing, ignore_index, (const int*)work, rowloss);
  });
  hipLaunchKernelGGL(ce_sum_kernel, dim3(1), dim3(kCeThreads), 0, st, rowloss, R, loss);
}

// Split form for the training step: the forward keeps only the per-row log-sum-exp (one pass
// over the logits: running max and rescaled exp-sum per thread, merged per wave and block), the
// backward writes grad = (softmax - target) * g / n straight from the logits with the upstream
// gradient g read on the device — so no [R][V] gradient is written in the forward and then
// rescaled by a separate elementwise pass (BERT-base MLM: 640 x 30528 logits).
__device__ __forceinline__ void lse_merge(float& m, float& s, float mo, float so) {
  const float mn = fmaxf(m, mo);
  if (mn == -INFINITY) return;  // both empty
  s = s * __expf(m - mn) + so * __expf(mo - mn);
  m = mn;
}

// MIX: the pair-target form (Mixup / CutMix).  Row r has the labels a = labels[r] and
// b = labels[R-1-r] with weights lambda = mix[0] and 1 - lambda, read on the device; every row
// counts (nvalid and ignore are unused).  lambda = 1 gives the hard-label result bit for bit:
// 1 * x[a] + 0 * x[b] is x[a], and (1 - eps) * (1 * [c==a] + 0 * [c==b]) is 1 - eps or 0.
template <class T, bool MIX = false>
__global__ __launch_bounds__(kCeThreads) void ce_fwd_kernel(const T* __restrict__ logits,
                                                     const int64_t* __restrict__ labels, int V,
                                                     int Vv, float eps, int64_t ignore,
                                                     const int* __restrict__ nvalid,
                                                     float* __restrict__ rowloss,
                                                     float* __restrict__ lse_out,
                                                     const float* __restrict__ mix = nullptr) {
  __shared__ float sh[3][kCeThreads / 64];
  const long row = blockIdx.x;
  const T* x = logits + row * V;
  float m = -INFINITY, s = 0.f, sx = 0.f;
  if ((V % kCeVec) == 0) {
    for (int c = threadIdx.x; c < V / kCeVec; c += kCeThreads) {
      float v[kCeVec];
      load8(x + c * kCeVec, v);
      float m8 = -INFINITY;
#pragma unroll
      for (int q = 0; q < kCeVec; ++q)
        if (c * kCeVec + q < Vv) {
          m8 = fmaxf(m8, v[q]);
          sx += v[q];
        }
      const float mn = fmaxf(m, m8);
      if (mn == -INFINITY) continue;
      float e = 0.f;
#pragma unroll
      for (int q = 0; q < kCeVec; ++q)
        if (c * kCeVec + q < Vv) e += __expf(v[q] - mn);
      s = s * __expf(m - mn) + e;
      m = mn;
    }
  } else {
    for (int c = threadIdx.x; c < Vv; c += kCeThreads) {
      const float v = (float)x[c];
      sx += v;
      lse_merge(m, s, v, 1.f);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float mo = __shfl_xor(m, o), so = __shfl_xor(s, o);
    lse_merge(m, s, mo, so);
    sx += __shfl_xor(sx, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sh[0][w] = m;
    sh[1][w] = s;
    sh[2][w] = sx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sh[0][0], S = sh[1][0], SX = sh[2][0];
    for (int i = 1; i < kCeThreads / 64; ++i) {
      lse_merge(M, S, sh[0][i], sh[1][i]);
      SX += sh[2][i];
    }
    float lse = M + __logf(S);
    // A NaN logit makes the row's log-sum-exp NaN, as in the fused kernel.  The merges above can
    // lose it (fmaxf skips a NaN, and a thread that has seen nothing else counts as empty); the
    // plain sum of the logits cannot.  (SX is also NaN with +inf and -inf in one row: lse
    // is NaN then anyway, from exp(inf - inf).)
    if (SX != SX) lse = SX;
    const int64_t lab = labels[row];
    bool valid = lab != ignore;
    float xl = 0.f;
    int n;
    if constexpr (MIX) {
      const int64_t lab2 = labels[(long)gridDim.x - 1 - row];
      const float lam = mix[0], om = 1.f - lam;
      // a label outside the classes reads nothing (its logit counts as 0)
      xl = lam * ce_label_logit(x, lab, Vv) + om * ce_label_logit(x, lab2, Vv);
      valid = true;
      n = (int)gridDim.x;
    } else {
      if (valid) xl = ce_label_logit(x, lab, Vv);
      n = nvalid[0];
    }
    float l = 0.f;
    if (valid) l = ce_row_loss(lse, xl, SX, Vv, eps);
    rowloss[row] = l / (float)max(1, n);
    lse_out[row] = lse;
  }
}

// grid (column blocks, rows): kCeVec columns per thread (V % kCeVec == 0) or 1
// the target of column col: eps / Vv + (1 - eps) on the label, or, pair-target, (1 - eps) times
// lambda on label a plus 1 - lambda on label b
template <bool MIX>
__device__ __forceinline__ float ce_target(int col, int64_t lab, int64_t lab2, float lam,
                                           float om, float base_t, float eps) {
  if constexpr (MIX)
    return base_t + (1.f - eps) * ((col == lab ? lam : 0.f) + (col == lab2 ? om : 0.f));
  else
    return base_t + (col == lab ? 1.f - eps : 0.f);
}

template <class T, bool VEC, bool MIX = false>
__global__ __launch_bounds__(kCeThreads) void ce_bwd_kernel(const T* __restrict__ logits,
                                                     const int64_t* __restrict__ labels,
                                                     const float* __restrict__ lse,
                                                     const int* __restrict__ nvalid,
                                                     const float* __restrict__ gout,
                                                     T* __restrict__ grad, int R, int V, int Vv,
                                                     float eps, int64_t ignore,
                                                     const float* __restrict__ mix = nullptr) {
  const int c = blockIdx.x * kCeThreads + threadIdx.x;
  if (c >= (VEC ? V / kCeVec : V)) return;
  const float gs = gout[0] / (float)max(1, MIX ? R : nvalid[0]), base_t = eps / (float)Vv;
  float lam = 1.f, om = 0.f;
  if constexpr (MIX) {
    lam = mix[0];
    om = 1.f - lam;
  }
  for (long row = blockIdx.y; row < R; row += gridDim.y) {  // (grid.y is capped at kCeBwdMaxGridRows)
  const int64_t lab = labels[row];
  const int64_t lab2 = MIX ? labels[R - 1 - row] : lab;
  const float scale = (MIX || lab != ignore) ? gs : 0.f;
  const float l = lse[row];
  if constexpr (VEC) {
    float v[kCeVec];
    load8(logits + row * V + c * kCeVec, v);
#pragma unroll
    for (int q = 0; q < kCeVec; ++q) {
      const int col = c * kCeVec + q;
      const float t = ce_target<MIX>(col, lab, lab2, lam, om, base_t, eps);
      v[q] = col < Vv ? (__expf(v[q] - l) - t) * scale : 0.f;
    }
    store8(grad + row * V + c * kCeVec, v);
  } else {
    const float t = ce_target<MIX>(c, lab, lab2, lam, om, base_t, eps);
    grad[row * V + c] = (T)(c < Vv ? (__expf((float)logits[row * V + c] - l) - t) * scale : 0.f);
  }
  }
}

// mix == null: hard labels (the valid rows are counted first); else the pair-target form
void cross_entropy_fwd(const void* logits, const int64_t* labels, const float* mix, float* loss,
                       int R, int V, float smoothing, int64_t ignore_index, int* work,
                       hipStream_t st, bool f32, int Vv) {
  if (Vv <= 0 || Vv > V) Vv = V;
  float* rowloss = reinterpret_cast<float*>(work + 4);
  float* lse = rowloss + R;
  if (mix == nullptr)
    hipLaunchKernelGGL(ce_count_kernel, dim3(1), dim3(kCeThreads), 0, st, labels, R, ignore_index, work);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    dispatch_bool(mix != nullptr, [&](auto mix_c) {
      constexpr bool MIX = decltype(mix_c)::value;
      hipLaunchKernelGGL((ce_fwd_kernel<T, MIX>), dim3(R), dim3(kCeThreads), 0, st, (const T*)logits,
                         labels, V, Vv, smoothing, MIX ? (int64_t)0 : ignore_index,
                         MIX ? (const int*)nullptr : (const int*)work, rowloss, lse, mix);
    });
  });
  hipLaunchKernelGGL(ce_sum_kernel, dim3(1), dim3(kCeThreads), 0, st, rowloss, R, loss);
}

void cross_entropy_bwd(const void* logits, const int64_t* labels, const float* mix,
                       const int* work, const float* gout, void* grad, int R, int V,
                       float smoothing, int64_t ignore_index, hipStream_t st, bool f32, int Vv) {
  if (Vv <= 0 || Vv > V) Vv = V;
  const float* lse = reinterpret_cast<const float*>(work + 4) + R;
  const bool vec = V % kCeVec == 0;
  const dim3 g((unsigned)(((vec ? V / kCeVec : V) + kCeThreads - 1) / kCeThreads),
               (unsigned)std::min(R, kCeBwdMaxGridRows));
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    dispatch_bool(vec, [&](auto vec_c) {
      dispatch_bool(mix != nullptr, [&](auto mix_c) {
        constexpr bool MIX = decltype(mix_c)::value;
        hipLaunchKernelGGL((ce_bwd_kernel<T, decltype(vec_c)::value, MIX>), g, dim3(kCeThreads), 0, st,
                           (const T*)logits, labels, lse, MIX ? (const int*)nullptr : work, gout,
                           (T*)grad, R, V, Vv, smoothing, MIX ? (int64_t)0 : ignore_index, mix);
      });
    });
  });
}

// ------------------------------------------------------------------------------ evaluation
// Top-1 correct count (the reference's eval loop: argmax over classes == label, summed): one
// wave per row, first maximal index wins (torch.argmax's tie rule), NaN counts as maximal; the
// per-block count is one integer atomic into *correct (order-independent, so deterministic).
template <class T>
__global__ __launch_bounds__(64 * kTop1RowsPerBlock) void top1_correct_kernel(const T* __restrict__ logits,
                                                           const int64_t* __restrict__ labels,
                                                           int R, int V, int* __restrict__ correct) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * kTop1RowsPerBlock + wave;
  int hit = 0;
  if (row < R) {
    const T* x = logits + (long)row * V;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int c = lane; c < V; c += 64) {
      const float v = (float)x[c];
      if (v > best || (v != v && best == best)) {  // strictly greater keeps the first index
        best = v;
        arg = c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oa = __shfl_xor(arg, o);
      const bool onan = ob != ob, mnan = best != best;
      // (two NaNs are equal: the lower index wins, as between two equal numbers)
      if ((onan && !mnan) ||
          (onan == mnan && (ob > best || ((onan || ob == best) && oa < arg)))) {
        best = ob;
        arg = oa;
      }
    }
    // no column was greater than -inf (a row of -inf only): all are equal, the first wins
    if (arg == 0x7fffffff && V > 0) arg = 0;
    hit = (lane == 0 && (int64_t)arg == labels[row]) ? 1 : 0;
  }
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  if (hit) atomicAdd(&cnt, 1);
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(correct, cnt);
}

void top1_correct(const void* logits, const int64_t* labels, int R, int V, int* correct,
                  hipStream_t st, bool f32) {
  dim3 g((R + kTop1RowsPerBlock - 1) / kTop1RowsPerBlock);
  dispatch_act(f32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(top1_correct_kernel<T>, g, dim3(64 * kTop1RowsPerBlock), 0, st, (const T*)logits, labels, R, V,
                       correct);
  });
}

}  // namespace mipipe
