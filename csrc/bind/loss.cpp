// Loss and evaluation entries of mipipe._C: the cross-entropy family (kernels/loss.hip), the
// top-1 count and the evaluation statistics (kernels/eval_stats.hip).  ce_args (common.hpp) is
// the one check of their logits / labels / work / gout operands.
#include "bind/common.hpp"

namespace mipipe_bind {
namespace {

// Split cross-entropy (training step): forward -> (loss, work = [count | row losses | row lse]),
// backward -> grad from the saved logits and the upstream gradient (a device scalar).
// mix (Mixup / CutMix): the pair-target form — row r is labelled labels[r] with weight mix[0] and
// labels[R-1-r] with weight 1 - mix[0]; every row counts, so there is no ignore_index.
std::tuple<Tensor, Tensor> ce_fwd(const Tensor& logits, const Tensor& labels, const Tensor* mix,
                                  double smoothing, int64_t ignore_index, int64_t valid_cols) {
  const CeArgs a = ce_args(logits, labels, valid_cols);
  if (mix != nullptr) check_mix(*mix, logits);
  c10::DeviceGuard g(logits.device());
  auto loss = torch::empty({}, logits.options().dtype(at::kFloat));
  auto work = torch::empty({4 + 2 * a.R}, logits.options().dtype(at::kInt));
  if (mix != nullptr && (a.R == 0 || a.V == 0)) return {loss.zero_(), work};
  mipipe::cross_entropy_fwd(logits.data_ptr(), labels.data_ptr<int64_t>(),
                            mix != nullptr ? mix->data_ptr<float>() : nullptr,
                            loss.data_ptr<float>(), (int)a.R, (int)a.V, (float)smoothing,
                            ignore_index, work.data_ptr<int>(), stream(), is_f32(logits),
                            (int)a.Vv);
  return {loss, work};
}

Tensor ce_bwd(const Tensor& logits, const Tensor& labels, const Tensor* mix, const Tensor& work,
              const Tensor& gout, double smoothing, int64_t ignore_index, int64_t valid_cols) {
  const CeArgs a = ce_args(logits, labels, valid_cols, work, gout);
  if (mix != nullptr) check_mix(*mix, logits);
  c10::DeviceGuard g(logits.device());
  auto grad = torch::empty_like(logits);
  if (mix != nullptr && (a.R == 0 || a.V == 0)) return grad;
  mipipe::cross_entropy_bwd(logits.data_ptr(), labels.data_ptr<int64_t>(),
                            mix != nullptr ? mix->data_ptr<float>() : nullptr,
                            work.data_ptr<int>(), gout.data_ptr<float>(), grad.data_ptr(),
                            (int)a.R, (int)a.V, (float)smoothing, ignore_index, stream(),
                            is_f32(logits), (int)a.Vv);
  return grad;
}

std::tuple<Tensor, Tensor> cross_entropy_fwd(Tensor logits, Tensor labels, double smoothing,
                                             int64_t ignore_index, int64_t valid_cols) {
  return ce_fwd(logits, labels, nullptr, smoothing, ignore_index, valid_cols);
}

Tensor cross_entropy_bwd(Tensor logits, Tensor labels, Tensor work, Tensor gout, double smoothing,
                         int64_t ignore_index, int64_t valid_cols) {
  return ce_bwd(logits, labels, nullptr, work, gout, smoothing, ignore_index, valid_cols);
}

std::tuple<Tensor, Tensor> cross_entropy_mixed_fwd(Tensor logits, Tensor labels, Tensor mix,
                                                   double smoothing, int64_t valid_cols) {
  return ce_fwd(logits, labels, &mix, smoothing, 0, valid_cols);
}

Tensor cross_entropy_mixed_bwd(Tensor logits, Tensor labels, Tensor mix, Tensor work, Tensor gout,
                               double smoothing, int64_t valid_cols) {
  return ce_bwd(logits, labels, &mix, work, gout, smoothing, 0, valid_cols);
}

// The fused form (loss and gradient in one pass over the logits): the tests' cross-check of the
// split form.
std::tuple<Tensor, Tensor> cross_entropy_fwd_bwd(Tensor logits, Tensor labels, double smoothing,
                                                 int64_t ignore_index, int64_t valid_cols) {
  const CeArgs a = ce_args(logits, labels, valid_cols);
  c10::DeviceGuard g(logits.device());
  auto loss = torch::empty({}, logits.options().dtype(at::kFloat));
  auto grad = torch::empty_like(logits);
  auto work = torch::empty({4 + a.R}, logits.options().dtype(at::kInt));  // count + row losses
  mipipe::cross_entropy_fwd_bwd(logits.data_ptr(), labels.data_ptr<int64_t>(), loss.data_ptr<float>(),
                                grad.data_ptr(), (int)a.R, (int)a.V, (float)smoothing, ignore_index,
                                work.data_ptr<int>(), stream(), is_f32(logits), (int)a.Vv);
  return {loss, grad};
}

// number of rows whose argmax equals the label, accumulated into an int32 device counter
Tensor top1_correct(Tensor logits, Tensor labels, optional<Tensor> out) {
  const CeArgs a = ce_args(logits, labels, -1, "top1");
  c10::DeviceGuard g(logits.device());
  Tensor o;
  if (out.has_value()) {
    check_cuda(*out, "out");
    TORCH_CHECK(out->scalar_type() == at::kInt && out->numel() == 1, "out must be one int32");
    o = *out;
  } else {
    o = torch::zeros({1}, logits.options().dtype(at::kInt));
  }
  if (a.R > 0)
    mipipe::top1_correct(logits.data_ptr(), labels.data_ptr<int64_t>(), (int)a.R, (int)a.V,
                         o.data_ptr<int>(), stream(), is_f32(logits));
  return o;
}

// Evaluation statistics of one batch (eval_stats.hip) accumulated into device buffers: counters
// int64 [8], confusion int32 [Vv, Vv] (optional), hist int64 [3, bins] (optional, 1 <= bins <= 64).
void eval_stats(Tensor logits, Tensor labels, Tensor counters, optional<Tensor> confusion,
                optional<Tensor> hist, int64_t k, int64_t ignore_index, int64_t valid_cols) {
  const CeArgs a = ce_args(logits, labels, valid_cols, "eval_stats");
  const int64_t R = a.R, V = a.V, Vv = a.Vv;
  check_cuda(counters, "counters");
  c10::DeviceGuard g(logits.device());
  TORCH_CHECK(counters.scalar_type() == at::kLong && counters.numel() == 8 &&
              counters.device() == logits.device(),
              "counters must be int64 [8] on the logits' device");
  TORCH_CHECK(R < (1ll << 31) - 4 && V < (1ll << 31), "eval_stats: logits too large");
  TORCH_CHECK(k >= 1 && k <= Vv, "k must be in [1, ", Vv, "], got ", k);
  int* cm = nullptr;
  if (confusion.has_value()) {
    check_cuda(*confusion, "confusion");
    TORCH_CHECK(confusion->scalar_type() == at::kInt && confusion->dim() == 2 &&
                confusion->size(0) == Vv && confusion->size(1) == Vv &&
                confusion->device() == logits.device(),
                "confusion must be int32 [", Vv, ", ", Vv, "] on the logits' device");
    cm = confusion->data_ptr<int>();
  }
  int64_t* hp = nullptr;
  int64_t bins = 1;
  if (hist.has_value()) {
    check_cuda(*hist, "hist");
    TORCH_CHECK(hist->scalar_type() == at::kLong && hist->dim() == 2 && hist->size(0) == 3 &&
                hist->size(1) >= 1 && hist->size(1) <= 64 && hist->device() == logits.device(),
                "hist must be int64 [3, bins] with 1 <= bins <= 64 on the logits' device");
    bins = hist->size(1);
    hp = hist->data_ptr<int64_t>();
  }
  if (R > 0)
    mipipe::eval_stats(logits.data_ptr(), labels.data_ptr<int64_t>(), (int)R, (int)V, (int)Vv,
                       (int)k, ignore_index, (int)bins, counters.data_ptr<int64_t>(), hp, cm,
                       stream(), is_f32(logits));
}

}  // namespace

void bind_loss(py::module& m) {
  // launch constants of loss.hip (launchers.hpp), for the edge tests
  m.attr("CE_THREADS") = mipipe::kCeThreads;
  m.attr("CE_VEC") = mipipe::kCeVec;
  m.attr("CE_BWD_MAX_GRID_ROWS") = mipipe::kCeBwdMaxGridRows;
  m.attr("TOP1_ROWS_PER_BLOCK") = mipipe::kTop1RowsPerBlock;
  m.def("cross_entropy_fwd", &cross_entropy_fwd, py::arg("logits"), py::arg("labels"),
        py::arg("smoothing") = 0.0, py::arg("ignore_index") = -100, py::arg("valid_cols") = -1);
  m.def("cross_entropy_bwd", &cross_entropy_bwd, py::arg("logits"), py::arg("labels"),
        py::arg("work"), py::arg("gout"), py::arg("smoothing") = 0.0,
        py::arg("ignore_index") = -100, py::arg("valid_cols") = -1);
  m.def("cross_entropy_fwd_bwd", &cross_entropy_fwd_bwd, py::arg("logits"), py::arg("labels"),
        py::arg("smoothing"), py::arg("ignore_index"), py::arg("valid_cols") = -1);
  m.def("cross_entropy_mixed_fwd", &cross_entropy_mixed_fwd, py::arg("logits"), py::arg("labels"),
        py::arg("mix"), py::arg("smoothing") = 0.0, py::arg("valid_cols") = -1);
  m.def("cross_entropy_mixed_bwd", &cross_entropy_mixed_bwd, py::arg("logits"), py::arg("labels"),
        py::arg("mix"), py::arg("work"), py::arg("gout"), py::arg("smoothing") = 0.0,
        py::arg("valid_cols") = -1);
  m.def("top1_correct", &top1_correct, py::arg("logits"), py::arg("labels"),
        py::arg("out") = py::none());
  m.def("eval_stats", &eval_stats, py::arg("logits"), py::arg("labels"), py::arg("counters"),
        py::arg("confusion") = py::none(), py::arg("hist") = py::none(), py::arg("k") = 5,
        py::arg("ignore_index") = -100, py::arg("valid_cols") = -1);
}

}  // namespace mipipe_bind
