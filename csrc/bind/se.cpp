// Squeeze-excitation / Hardswish entries of mipipe._C (kernels/se.hip): BatchNorm apply +
// ReLU / Hardswish with the global average pool in the same pass, its two-pass backward with the
// pool's gradient as an addend, and the Hardsigmoid gate multiply both ways.
#include "bind/common.hpp"

namespace mipipe_bind {
namespace {

inline void check_aligned16(const Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

struct SeArgs {
  int N, HW, C;
};
// x [N, H, W, C] NHWC bf16 / fp32; C % 8 == 0, non-empty, < 2^31 elements, 16-byte aligned
SeArgs se_args(const Tensor& x, const char* name) {
  check_act(x, name);
  TORCH_CHECK(x.dim() == 4, name, " must be [N, H, W, C], got ", x.dim(), " dimensions");
  TORCH_CHECK(x.numel() > 0, name, " must not be empty");
  const int64_t C = x.size(3);
  TORCH_CHECK(C % 8 == 0, "the squeeze-excitation kernels need C % 8 == 0, got ", C);
  TORCH_CHECK(x.numel() < (1ll << 31), name, " must have fewer than 2^31 elements");
  check_aligned16(x, name);
  return {(int)x.size(0), (int)(x.size(1) * x.size(2)), (int)C};
}
void check_like(const Tensor& t, const Tensor& ref, const char* name) {
  check_same(t, ref, name);
  TORCH_CHECK(t.sizes() == ref.sizes(), name, " must have the shape ", ref.sizes(), ", got ",
              t.sizes());
  TORCH_CHECK(t.device() == ref.device(), name, " must be on the device of the other operands");
  check_aligned16(t, name);
}
// fp32 vector of n elements on ref's device, read 8 floats at a time
const float* vec_ptr(const Tensor& t, int64_t n, const Tensor& ref, const char* name) {
  check_vec(t, n, name);
  TORCH_CHECK(t.device() == ref.device(), name, " must be on the device of the other operands");
  check_aligned16(t, name);
  return t.data_ptr<float>();
}
const float* opt_vec_ptr(const optional<Tensor>& t, int64_t n, const Tensor& ref,
                         const char* name) {
  return t.has_value() ? vec_ptr(*t, n, ref, name) : nullptr;
}
int check_se_act(int64_t act) {
  TORCH_CHECK(act == mipipe::kSeActRelu || act == mipipe::kSeActHardswish,
              "act must be SE_ACT_RELU or SE_ACT_HARDSWISH, got ", act);
  return (int)act;
}
// gate [N, C] (or [N, 1, 1, C]) in x's dtype
void check_gate(const Tensor& gate, const Tensor& x, const SeArgs& a) {
  check_same(gate, x, "gate");
  TORCH_CHECK(gate.numel() == (int64_t)a.N * a.C && gate.size(-1) == a.C && gate.size(0) == a.N,
              "gate must be [N, C] = [", a.N, ", ", a.C, "], got ", gate.sizes());
  TORCH_CHECK(gate.device() == x.device(), "gate must be on the device of the other operands");
  check_aligned16(gate, "gate");
}
// the [N, slices, C] partial rows of a per-sample sum (none when a slice is a whole sample)
Tensor slice_ws(const SeArgs& a, const Tensor& like) {
  const int S = mipipe::se_slices(a.N, a.HW, a.C).slices;
  return S > 1 ? torch::empty({a.N, S, a.C}, like.options().dtype(at::kFloat)) : Tensor();
}

// -> (z, pm): z = T(act(y * scale + bias)), pm [N, C] fp32 = mean over (h, w) of the stored z
std::tuple<Tensor, optional<Tensor>> bn_act_pool_fwd(Tensor y, Tensor scale, Tensor bias,
                                                     int64_t act, bool want_pool) {
  const SeArgs a = se_args(y, "y");
  const int ac = check_se_act(act);
  const float* ps = vec_ptr(scale, a.C, y, "scale");
  const float* pb = vec_ptr(bias, a.C, y, "bias");
  c10::DeviceGuard g(y.device());
  auto z = torch::empty_like(y);
  optional<Tensor> pm;
  Tensor ws;
  if (want_pool) {
    pm = torch::empty({a.N, a.C}, y.options().dtype(at::kFloat));
    ws = slice_ws(a, y);
  }
  mipipe::bn_act_pool_fwd(y.data_ptr(), ps, pb, z.data_ptr(),
                          want_pool ? pm->data_ptr<float>() : nullptr, wsp(ws), a.N, a.HW, a.C, ac,
                          is_f32(y), stream());
  return {z, pm};
}

struct BwdPtrs {
  const float *scale, *bias, *mean, *invstd, *dpm;
};
BwdPtrs bwd_args(const Tensor& dz, const Tensor& y, const SeArgs& a, const Tensor& scale,
                 const Tensor& bias, const Tensor& mean, const Tensor& invstd,
                 const optional<Tensor>& dpm) {
  check_like(dz, y, "dz");
  BwdPtrs p;
  p.scale = vec_ptr(scale, a.C, y, "scale");
  p.bias = vec_ptr(bias, a.C, y, "bias");
  p.mean = vec_ptr(mean, a.C, y, "mean");
  p.invstd = vec_ptr(invstd, a.C, y, "invstd");
  p.dpm = opt_vec_ptr(dpm, (int64_t)a.N * a.C, y, "dpm");
  return p;
}

// -> (sum g, sum g * xhat), fp32 [C] each
std::tuple<Tensor, Tensor> bn_act_pool_bwd_reduce(Tensor dz, Tensor y, Tensor scale, Tensor bias,
                                                  Tensor mean, Tensor invstd, int64_t act,
                                                  optional<Tensor> dpm) {
  const SeArgs a = se_args(y, "y");
  const int ac = check_se_act(act);
  const BwdPtrs p = bwd_args(dz, y, a, scale, bias, mean, invstd, dpm);
  c10::DeviceGuard g(y.device());
  auto o = y.options().dtype(at::kFloat);
  auto sums = torch::empty({2, a.C}, o);
  auto ws = torch::empty({2, (int64_t)mipipe::se_reduce_rows(a.N, a.HW, a.C), a.C}, o);
  mipipe::bn_act_pool_bwd_reduce(dz.data_ptr(), y.data_ptr(), p.scale, p.bias, p.mean, p.invstd,
                                 p.dpm, ws.data_ptr<float>(), sums.data_ptr<float>(),
                                 sums.data_ptr<float>() + a.C, a.N, a.HW, a.C, ac, is_f32(y),
                                 stream());
  return {sums[0], sums[1]};
}

Tensor bn_act_pool_bwd_apply(Tensor dz, Tensor y, Tensor scale, Tensor bias, Tensor mean,
                             Tensor invstd, Tensor gamma, int64_t act, optional<Tensor> dpm,
                             optional<Tensor> sum_g, optional<Tensor> sum_gx) {
  const SeArgs a = se_args(y, "y");
  const int ac = check_se_act(act);
  const BwdPtrs p = bwd_args(dz, y, a, scale, bias, mean, invstd, dpm);
  const float* pg = vec_ptr(gamma, a.C, y, "gamma");
  TORCH_CHECK(sum_g.has_value() == sum_gx.has_value(), "pass both sums or none");
  const float* psg = opt_vec_ptr(sum_g, a.C, y, "sum_g");
  const float* psgx = opt_vec_ptr(sum_gx, a.C, y, "sum_gx");
  c10::DeviceGuard g(y.device());
  auto dy = torch::empty_like(y);
  mipipe::bn_act_pool_bwd_apply(dz.data_ptr(), y.data_ptr(), p.scale, p.bias, p.mean, p.invstd,
                                pg, p.dpm, psg, psgx, dy.data_ptr(), a.N, a.HW, a.C, ac, is_f32(y),
                                stream());
  return dy;
}

Tensor se_scale_fwd(Tensor z, Tensor gate) {
  const SeArgs a = se_args(z, "z");
  check_gate(gate, z, a);
  c10::DeviceGuard g(z.device());
  auto out = torch::empty_like(z);
  mipipe::se_scale_fwd(z.data_ptr(), gate.data_ptr(), out.data_ptr(), a.N, a.HW, a.C, is_f32(z),
                       stream());
  return out;
}

// -> (dz, dgate); dgate in gate's shape and dtype
std::tuple<Tensor, Tensor> se_scale_bwd(Tensor dout, Tensor z, Tensor gate) {
  const SeArgs a = se_args(z, "z");
  check_like(dout, z, "dout");
  check_gate(gate, z, a);
  c10::DeviceGuard g(z.device());
  auto dz = torch::empty_like(z);
  auto dgate = torch::empty_like(gate);
  Tensor ws = slice_ws(a, z);
  mipipe::se_scale_bwd(dout.data_ptr(), z.data_ptr(), gate.data_ptr(), dz.data_ptr(),
                       dgate.data_ptr(), wsp(ws), a.N, a.HW, a.C, is_f32(z), stream());
  return {dz, dgate};
}

// (threads per row, rows per block pass, rows per slice, slices per sample, grid.y)
std::tuple<int, int, int, int, int> se_slices(int64_t N, int64_t HW, int64_t C) {
  TORCH_CHECK(N >= 1 && HW >= 1 && C >= 8 && C % 8 == 0 && N * HW * C < (1ll << 31),
              "se_slices: N, HW >= 1, C % 8 == 0, fewer than 2^31 elements");
  const mipipe::SeSlices s = mipipe::se_slices((int)N, (int)HW, (int)C);
  return {s.tpr, s.rpb, s.rows, s.slices, s.cy};
}

}  // namespace

void bind_se(py::module& m) {
  m.def("bn_act_pool_fwd", &bn_act_pool_fwd, py::arg("y"), py::arg("scale"), py::arg("bias"),
        py::arg("act"), py::arg("want_pool") = false);
  m.def("bn_act_pool_bwd_reduce", &bn_act_pool_bwd_reduce, py::arg("dz"), py::arg("y"),
        py::arg("scale"), py::arg("bias"), py::arg("mean"), py::arg("invstd"), py::arg("act"),
        py::arg("dpm") = py::none());
  m.def("bn_act_pool_bwd_apply", &bn_act_pool_bwd_apply, py::arg("dz"), py::arg("y"),
        py::arg("scale"), py::arg("bias"), py::arg("mean"), py::arg("invstd"), py::arg("gamma"),
        py::arg("act"), py::arg("dpm") = py::none(), py::arg("sum_g") = py::none(),
        py::arg("sum_gx") = py::none());
  m.def("se_scale_fwd", &se_scale_fwd, py::arg("z"), py::arg("gate"));
  m.def("se_scale_bwd", &se_scale_bwd, py::arg("dout"), py::arg("z"), py::arg("gate"));
  m.def("se_slices", &se_slices, py::arg("N"), py::arg("HW"), py::arg("C"));
  m.attr("SE_THREADS") = mipipe::kSeThreads;
  m.attr("SE_ROW_U") = mipipe::kSeRowU;
  m.attr("SE_TARGET_BLOCKS") = mipipe::kSeTargetBlocks;
  m.attr("SE_MAX_BLOCKS") = mipipe::kSeMaxBlocks;
  m.attr("SE_REDUCE_BLOCKS") = mipipe::kSeReduceBlocks;
  m.attr("SE_ACT_RELU") = mipipe::kSeActRelu;
  m.attr("SE_ACT_HARDSWISH") = mipipe::kSeActHardswish;
}

}  // namespace mipipe_bind
