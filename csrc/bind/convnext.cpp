// ConvNeXt entries of mipipe._C (kernels/dwconv7.hip): the 7x7 depthwise convolution (forward,
// data-grad with the residual stream's addend, atomics-free weight-grad) and the block's closing
// layer scale + stochastic depth + residual.
#include "bind/common.hpp"
#include "kernels/convnext.hpp"

namespace mipipe_bind {
namespace {

inline void check_aligned16(const Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

struct Dw7Args {
  int N, H, W, C;
};
// x [N, H, W, C] NHWC bf16 / fp32; C % 8 == 0, C <= 2048, non-empty, < 2^31 elements
Dw7Args dw7_args(const Tensor& x, const char* name) {
  check_act(x, name);
  TORCH_CHECK(x.dim() == 4, name, " must be [N, H, W, C], got ", x.dim(), " dimensions");
  const int64_t C = x.size(3);
  TORCH_CHECK(x.numel() > 0, name, " must not be empty");
  TORCH_CHECK(C % 8 == 0, "dwconv7 needs C % 8 == 0, got ", C);
  TORCH_CHECK(C <= mipipe::kDw7MaxChannels, "dwconv7 needs C <= ", mipipe::kDw7MaxChannels,
              ", got ", C);
  TORCH_CHECK(x.numel() < (1ll << 31), "dwconv7: ", name, " must have fewer than 2^31 elements");
  check_aligned16(x, name);
  return {(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)C};
}
// the operand weight [C, 7, 7, 1] in x's dtype, on x's device
void check_dw7_weight(const Tensor& w, const Tensor& x, int C) {
  check_same(w, x, "w");
  TORCH_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == 7 && w.size(2) == 7 && w.size(3) == 1,
              "w must be [", C, ", 7, 7, 1], got ", w.sizes());
  TORCH_CHECK(w.device() == x.device(), "w must be on the device of the other operands");
  check_aligned16(w, "w");
}
void check_like(const Tensor& t, const Tensor& ref, const char* name) {
  check_same(t, ref, name);
  TORCH_CHECK(t.sizes() == ref.sizes(), name, " must have the shape ", ref.sizes(), ", got ",
              t.sizes());
  TORCH_CHECK(t.device() == ref.device(), name, " must be on the device of the other operands");
  check_aligned16(t, name);
}
// an fp32 accumulator of n elements on ref's device (the flat-gradient view of a parameter).
// No alignment is asked of it: the fixed-order finish (det_sum_rows) reads and writes it one
// float at a time.
float* acc_ptr(const optional<Tensor>& t, int64_t n, const Tensor& ref, const char* name) {
  if (!t.has_value()) return nullptr;
  check_vec(*t, n, name);
  TORCH_CHECK(t->device() == ref.device(), name, " must be on the device of the other operands");
  return t->data_ptr<float>();
}
const uint32_t* seed_counter(const optional<Tensor>& t, const Tensor& ref) {
  if (!t.has_value()) return nullptr;
  check_cuda(*t, "seed_dev");
  TORCH_CHECK(t->scalar_type() == at::kInt && t->numel() >= 1 && t->device() == ref.device(),
              "seed_dev must be an int32 device counter on the device of the other operands");
  return reinterpret_cast<const uint32_t*>(t->data_ptr<int>());
}

Tensor dwconv7_fwd(Tensor x, Tensor w, optional<Tensor> bias) {
  const Dw7Args a = dw7_args(x, "x");
  check_dw7_weight(w, x, a.C);
  const float* pb = acc_ptr(bias, a.C, x, "bias");
  if (pb != nullptr) check_aligned16(*bias, "bias");
  c10::DeviceGuard g(x.device());
  auto y = torch::empty_like(x);
  mipipe::dwconv7_fwd(x.data_ptr(), w.data_ptr(), pb, nullptr, y.data_ptr(), a.N, a.H, a.W, a.C,
                      false, is_f32(x), stream());
  return y;
}

// dx = T(conv(dy, w mirrored) + addend): the addend (dx's shape) is the residual stream's gradient
Tensor dwconv7_dgrad(Tensor dy, Tensor w, optional<Tensor> addend) {
  const Dw7Args a = dw7_args(dy, "dy");
  check_dw7_weight(w, dy, a.C);
  if (addend.has_value()) check_like(*addend, dy, "addend");
  c10::DeviceGuard g(dy.device());
  auto dx = torch::empty_like(dy);
  mipipe::dwconv7_fwd(dy.data_ptr(), w.data_ptr(), nullptr, ptr_or_null(addend), dx.data_ptr(),
                      a.N, a.H, a.W, a.C, true, is_f32(dy), stream());
  return dx;
}

// dw [C, 1, 7, 7] += sum dy * x(shifted), db [C] += sum dy, both fp32: ACCUMULATED into dw_acc /
// db_acc (e.g. the flat-gradient views) and returned as None, or into new zeroed tensors
std::tuple<optional<Tensor>, optional<Tensor>> dwconv7_wgrad(Tensor dy, Tensor x,
                                                             optional<Tensor> dw_acc,
                                                             optional<Tensor> db_acc) {
  const Dw7Args a = dw7_args(x, "x");
  check_like(dy, x, "dy");
  c10::DeviceGuard g(x.device());
  auto o = x.options().dtype(at::kFloat);
  optional<Tensor> dw, db;
  float* pw = acc_ptr(dw_acc, (int64_t)a.C * 49, x, "dw");
  float* pb = acc_ptr(db_acc, a.C, x, "dbias");
  if (pw == nullptr) {
    dw = torch::zeros({a.C, 1, 7, 7}, o);
    pw = dw->data_ptr<float>();
  }
  if (pb == nullptr) {
    db = torch::zeros({a.C}, o);
    pb = db->data_ptr<float>();
  }
  const int64_t P = mipipe::dw7_wgrad_rows(a.N, a.H, a.W, a.C, is_f32(x));
  auto ws = torch::empty({P, (int64_t)a.C * 50}, o);  // [P, C*49] weight rows | [P, C] bias rows
  float* ws_w = ws.data_ptr<float>();
  mipipe::dwconv7_wgrad(dy.data_ptr(), x.data_ptr(), ws_w, ws_w + P * a.C * 49, pw, pb, a.N, a.H,
                        a.W, a.C, is_f32(x), stream());
  return {dw, db};
}

struct SrArgs {
  int64_t R, C, HW;
};
SrArgs sr_args(const Tensor& f, const Tensor& gamma, int64_t hw, double p) {
  check_act(f, "f");
  TORCH_CHECK(f.dim() >= 2, "f must be [..., C]");
  TORCH_CHECK(f.numel() > 0, "f must not be empty");
  const int64_t C = f.size(-1), R = f.numel() / C;
  TORCH_CHECK(C % 8 == 0, "scale_residual needs C % 8 == 0, got ", C);
  TORCH_CHECK(f.numel() < (1ll << 31), "scale_residual: f must have fewer than 2^31 elements");
  TORCH_CHECK(hw >= 1 && R % hw == 0, "the rows (", R, ") are not whole samples of ", hw);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "the drop probability must be in [0, 1), got ", p);
  check_vec(gamma, C, "gamma");
  TORCH_CHECK(gamma.device() == f.device(), "gamma must be on the device of the other operands");
  check_aligned16(f, "f");
  check_aligned16(gamma, "gamma");
  return {R, C, hw};
}
mipipe::PathDrop path_drop(double p, int64_t seed, const optional<Tensor>& seed_dev,
                           const Tensor& ref) {
  mipipe::PathDrop d{1.f, 0u, 0u, nullptr};
  if (p > 0.0) {
    d.scale = (float)(1.0 / (1.0 - p));
    d.thr = mipipe::drop_threshold_host(p);
    d.seed = (uint32_t)seed;
    d.seed_dev = seed_counter(seed_dev, ref);
  }
  return d;
}

// out = T(res + (f * gamma[c]) * s_n), s_n = keep_n / (1 - p) by sample n = row / hw
Tensor scale_residual_fwd(Tensor f, Tensor res, Tensor gamma, int64_t hw, double p, int64_t seed,
                          optional<Tensor> seed_dev) {
  const SrArgs a = sr_args(f, gamma, hw, p);
  check_like(res, f, "res");
  c10::DeviceGuard g(f.device());
  auto out = torch::empty_like(f);
  mipipe::scale_residual_fwd(f.data_ptr(), res.data_ptr(), gamma.data_ptr<float>(), out.data_ptr(),
                             a.R, (int)a.C, (int)a.HW, path_drop(p, seed, seed_dev, f), is_f32(f),
                             stream());
  return out;
}

// -> (df, dgamma, dbias).  dgamma is ACCUMULATED into dgamma_acc (returned as None) or a new zeroed
// tensor; dbias likewise when want_bias or dbias_acc is given, else not computed (None).
std::tuple<Tensor, optional<Tensor>, optional<Tensor>> scale_residual_bwd(
    Tensor dout, Tensor f, Tensor gamma, int64_t hw, double p, int64_t seed,
    optional<Tensor> seed_dev, optional<Tensor> dgamma_acc, optional<Tensor> dbias_acc,
    bool want_bias) {
  const SrArgs a = sr_args(f, gamma, hw, p);
  check_like(dout, f, "dout");
  c10::DeviceGuard g(f.device());
  auto o = f.options().dtype(at::kFloat);
  optional<Tensor> dg, db;
  float* pg = acc_ptr(dgamma_acc, a.C, f, "dgamma");
  float* pb = acc_ptr(dbias_acc, a.C, f, "dbias");
  if (pg == nullptr) {
    dg = torch::zeros({a.C}, o);
    pg = dg->data_ptr<float>();
  }
  if (pb == nullptr && want_bias) {
    db = torch::zeros({a.C}, o);
    pb = db->data_ptr<float>();
  }
  const int64_t P = mipipe::sr_bwd_rows(a.R, (int)a.C);
  auto ws = torch::empty({2 * P, a.C}, o);
  float* ws_g = ws.data_ptr<float>();
  auto df = torch::empty_like(f);
  mipipe::scale_residual_bwd(dout.data_ptr(), f.data_ptr(), gamma.data_ptr<float>(), df.data_ptr(),
                             ws_g, ws_g + P * a.C, pg, pb, a.R, (int)a.C, (int)a.HW,
                             path_drop(p, seed, seed_dev, f), is_f32(f), stream());
  return {df, dg, db};
}

}  // namespace

void bind_convnext(py::module& m) {
  m.def("dwconv7_fwd", &dwconv7_fwd, py::arg("x"), py::arg("w"), py::arg("bias") = py::none());
  m.def("dwconv7_dgrad", &dwconv7_dgrad, py::arg("dy"), py::arg("w"),
        py::arg("addend") = py::none());
  m.def("dwconv7_wgrad", &dwconv7_wgrad, py::arg("dy"), py::arg("x"), py::arg("dw") = py::none(),
        py::arg("dbias") = py::none());
  m.def("scale_residual_fwd", &scale_residual_fwd, py::arg("f"), py::arg("res"), py::arg("gamma"),
        py::arg("hw"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("seed_dev") = py::none());
  m.def("scale_residual_bwd", &scale_residual_bwd, py::arg("dout"), py::arg("f"),
        py::arg("gamma"), py::arg("hw"), py::arg("p") = 0.0, py::arg("seed") = 0,
        py::arg("seed_dev") = py::none(), py::arg("dgamma") = py::none(),
        py::arg("dbias") = py::none(), py::arg("want_bias") = false);
  m.attr("DW7_TILE_H") = mipipe::kDw7TileH;
  m.attr("DW7_TILE_W") = mipipe::kDw7TileW;
  m.attr("DW7_CHAN_BLOCK") = mipipe::dw7_chan_block(false);
  m.attr("DW7_CHAN_BLOCK_F32") = mipipe::dw7_chan_block(true);
  m.attr("DW7_MAX_CHANNELS") = mipipe::kDw7MaxChannels;
  m.attr("DW7_MAX_BLOCKS") = mipipe::kDw7MaxBlocks;
  m.attr("DW7_WGRAD_BLOCKS") = mipipe::kDw7WgradBlocks;
  m.attr("DW7_WGRAD_MIN_ROWS") = mipipe::kDw7WgradMinRows;
  m.attr("DW7_WGRAD_MAX_ROWS") = mipipe::kDw7WgradMaxRows;
  m.attr("SR_FWD_TILE") = mipipe::kSrFwdThreads * mipipe::kSrFwdItems;
  m.attr("SR_FWD_MAX_BLOCKS") = mipipe::kSrFwdMaxBlocks;
  m.attr("SR_BLOCK_ROWS") = mipipe::kSrBlockRows;
  m.attr("SR_MAX_BLOCKS") = mipipe::kSrMaxBlocks;
}

}  // namespace mipipe_bind
