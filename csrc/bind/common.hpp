// What every family file under csrc/bind/ shares: the current stream, the dtype / contiguity
// checks, and the argument checks that several entries make (the cross-entropy family, the record
// loaders' inputs, the mix descriptor), each written once.
//
// Every entry validates dtypes, contiguity and the shape constraints the kernels and their
// grids assume (NHWC, channels % 8 == 0, K % 8 == 0 ...) on the HOST before launching, so a bad
// call raises a Python error instead of faulting the GPU.  Outputs are allocated with the torch
// caching allocator and kernels run on the current HIP stream (graph-capturable).
#pragma once
// (torch/extension.h would also parse the whole C++ frontend, torch/all.h: about 20 s more per unit)
#include <torch/types.h>
#include <torch/csrc/utils/pybind.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <c10/core/DeviceGuard.h>
#include <pybind11/stl.h>

#include <string>
#include <vector>

#include "kernels/launchers.hpp"

namespace mipipe_bind {

using torch::Tensor;
using c10::optional;

inline hipStream_t stream() { return at::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(); }

inline void check_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
inline void check_bf16(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bfloat16, got ", t.scalar_type());
}
// activation tensors: bf16 (mixed precision) or fp32 (the reference's precision)
inline void check_act(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat, name,
              " must be bfloat16 or float32, got ", t.scalar_type());
}
inline void check_same(const Tensor& t, const Tensor& ref, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == ref.scalar_type(), name, " must be ", ref.scalar_type(),
              " like the other operands, got ", t.scalar_type());
}
inline bool is_f32(const Tensor& t) { return t.scalar_type() == at::kFloat; }
inline void check_f32(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32, got ", t.scalar_type());
}
inline void check_vec(const Tensor& t, int64_t C, const char* name) {
  check_f32(t, name);
  TORCH_CHECK(t.numel() == C, name, " must have ", C, " elements, got ", t.numel());
}
inline const void* ptr_or_null(const optional<Tensor>& t) {
  return t.has_value() ? t->data_ptr() : nullptr;
}
inline float* fptr(const optional<Tensor>& t, int64_t n) {
  if (!t.has_value()) return nullptr;
  check_vec(*t, n, "gradient accumulator");
  return t->data_ptr<float>();
}
// an on/off environment switch (unset: dflt); callers keep the result in a static: read once
inline bool env_flag(const char* name, bool dflt) {
  const char* v = getenv(name);
  return v == nullptr ? dflt : atoi(v) != 0;
}
// fp32 workspace of a split-K conv plan (n elements; n == 0: no split, undefined / null)
inline Tensor split_ws(long n, const Tensor& like) {
  return n > 0 ? torch::empty({n}, like.options().dtype(at::kFloat)) : Tensor();
}
inline float* wsp(const Tensor& t) { return t.defined() ? t.data_ptr<float>() : nullptr; }

// torch's pooling output size (ceil_mode: the last window must start inside input or left pad)
// A padded input shorter than the window has no output: C++ division truncates toward zero, so
// a negative numerator would give extent 1 instead of torch's error.
inline int pool_out(int L, int k, int s, int p, bool ceil_mode) {
  TORCH_CHECK(L + 2 * p >= k, "padded input (", L, " + 2*", p, ") is smaller than the pooling window ",
              k);
  int num = L + 2 * p - k;
  int o = (ceil_mode ? (num + s - 1) / s : num / s) + 1;
  if (ceil_mode && (o - 1) * s >= L + p) --o;
  return o;
}

// the device-side mix descriptor (mipipe/data/mix.py): fp32, >= 8 elements, on `ref`'s device
inline void check_mix(const Tensor& mix, const Tensor& ref) {
  check_f32(mix, "mix");
  TORCH_CHECK(mix.numel() >= 8, "mix must hold at least 8 elements, got ", mix.numel());
  TORCH_CHECK(mix.device() == ref.device(), "mix must be on the device of the other operands");
}

// ---- the cross-entropy family (and the metrics that read the same operands) -------------------
// logits [R, V] bf16 / fp32, contiguous, on the GPU; labels int64, contiguous, R of them, on the
// logits' device.  Vv: valid_cols clamped to [1, V] (<= 0: all V columns are classes).
struct CeArgs {
  int64_t R, V, Vv;
};
inline CeArgs ce_args(const Tensor& logits, const Tensor& labels, int64_t valid_cols = -1,
                      const char* what = "CE") {
  check_act(logits, "logits");
  check_cuda(labels, "labels");
  TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
  TORCH_CHECK(logits.dim() == 2 && labels.numel() == logits.size(0), what, " shape mismatch");
  TORCH_CHECK(labels.device() == logits.device(), "labels must be on the logits' device");
  const int64_t V = logits.size(1);
  return {logits.size(0), V, std::min<int64_t>(valid_cols > 0 ? valid_cols : V, V)};
}
// ... and what the split form's backward gets from its forward: work int32 [4 + 2R] (count | row
// losses | row lse) and the upstream gradient gout, one fp32 value, both on the logits' device
inline CeArgs ce_args(const Tensor& logits, const Tensor& labels, int64_t valid_cols,
                      const Tensor& work, const Tensor& gout) {
  const CeArgs a = ce_args(logits, labels, valid_cols);
  check_cuda(work, "work");
  TORCH_CHECK(work.scalar_type() == at::kInt && work.numel() == 4 + 2 * a.R,
              "CE work buffer mismatch");
  check_f32(gout, "gout");
  TORCH_CHECK(gout.numel() == 1 && gout.device() == logits.device() &&
              work.device() == logits.device(),
              "gout must be one value; every operand on the logits' device");
  return a;
}

// ---- the record loaders' inputs ---------------------------------------------------------------
// idx: the int64 sample indices of a batch of n, on `like`'s device
inline void check_sample_idx(const Tensor& idx, const Tensor& like, int64_t n) {
  check_cuda(idx, "idx");
  TORCH_CHECK(idx.scalar_type() == at::kLong, "idx must be int64, got ", idx.scalar_type());
  TORCH_CHECK(idx.device() == like.device(), "idx must be on the device of the other operands");
  TORCH_CHECK(idx.dim() == 1 && idx.size(0) == n, "idx must be [n]");
}
// rec [n, label_bytes + C*H*W] uint8 whole records (1 <= label_bytes <= 8; the caller has checked
// that C*H*W is in range) and their idx [n].  Returns n.
inline int64_t check_records(const Tensor& rec, const Tensor& idx, int64_t C, int64_t H, int64_t W,
                             int64_t label_bytes) {
  check_cuda(rec, "rec");
  TORCH_CHECK(rec.scalar_type() == at::kByte, "rec must be uint8, got ", rec.scalar_type());
  TORCH_CHECK(label_bytes >= 1 && label_bytes <= 8, "label_bytes must be in [1, 8]");
  TORCH_CHECK(rec.dim() == 2 && rec.size(1) == label_bytes + C * H * W, "rec must be [n, ",
              label_bytes + C * H * W, "] (label bytes + C*H*W)");
  check_sample_idx(idx, rec, rec.size(0));
  return rec.size(0);
}

}  // namespace mipipe_bind
