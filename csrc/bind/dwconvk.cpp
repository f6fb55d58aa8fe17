// Depthwise K x K entries of mipipe._C (kernels/dwconvk.hip): K in {3, 5}, stride in {1, 2}, pad
// (K - 1) / 2, NHWC, no bias: forward with BatchNorm's shifted statistics in the same pass,
// data-grad with an optional addend, atomics-free weight-grad.
#include "bind/common.hpp"

namespace mipipe_bind {
namespace {

inline void check_aligned16(const Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

struct DwkArgs {
  int N, H, W, C, Ho, Wo, k, s;
};
void check_ks(int64_t k, int64_t s) {
  TORCH_CHECK(k == 3 || k == 5, "dwconvk: the kernel size must be 3 or 5, got ", k);
  TORCH_CHECK(s == 1 || s == 2, "dwconvk: the stride must be 1 or 2, got ", s);
}
// t [N, h, w, C] NHWC bf16 / fp32; C % 8 == 0, non-empty, < 2^31 elements, 16-byte aligned
void check_nhwc(const Tensor& t, const char* name) {
  check_act(t, name);
  TORCH_CHECK(t.dim() == 4, name, " must be [N, H, W, C], got ", t.dim(), " dimensions");
  TORCH_CHECK(t.numel() > 0, name, " must not be empty");
  TORCH_CHECK(t.size(3) % 8 == 0, "dwconvk needs C % 8 == 0, got ", t.size(3));
  TORCH_CHECK(t.numel() < (1ll << 31), "dwconvk: ", name, " must have fewer than 2^31 elements");
  check_aligned16(t, name);
}
// x: the convolution's input
DwkArgs dwk_args(const Tensor& x, int64_t k, int64_t s) {
  check_ks(k, s);
  check_nhwc(x, "x");
  DwkArgs a{(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3), 0, 0, (int)k, (int)s};
  a.Ho = mipipe::dwk_out(a.H, a.k, a.s);
  a.Wo = mipipe::dwk_out(a.W, a.k, a.s);
  return a;
}
// the operand weight [C, K, K, 1] in ref's dtype, on its device; -> K
int64_t check_weight(const Tensor& w, const Tensor& ref) {
  check_same(w, ref, "w");
  const int64_t C = ref.size(3);
  TORCH_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == w.size(2) && w.size(3) == 1,
              "w must be [", C, ", K, K, 1], got ", w.sizes());
  TORCH_CHECK(w.device() == ref.device(), "w must be on the device of the other operands");
  check_aligned16(w, "w");
  return w.size(1);
}
// dy of a convolution with the arguments a
void check_dy(const Tensor& dy, const Tensor& ref, const DwkArgs& a) {
  check_same(dy, ref, "dy");
  check_nhwc(dy, "dy");
  TORCH_CHECK(dy.size(0) == a.N && dy.size(1) == a.Ho && dy.size(2) == a.Wo && dy.size(3) == a.C,
              "dy must be [", a.N, ", ", a.Ho, ", ", a.Wo, ", ", a.C, "], got ", dy.sizes());
  TORCH_CHECK(dy.device() == ref.device(), "dy must be on the device of the other operands");
}

// -> (y, ps, pss): y = T(conv(x, w)); with shift (fp32 [C]) also ps / pss [1, C] fp32, the sums
// of (y - shift) and its square over the STORED y, else None
std::tuple<Tensor, optional<Tensor>, optional<Tensor>> dwconvk_fwd(Tensor x, Tensor w,
                                                                   int64_t stride,
                                                                   optional<Tensor> shift) {
  check_nhwc(x, "x");
  const DwkArgs a = dwk_args(x, check_weight(w, x), stride);
  const float* psh = nullptr;
  if (shift.has_value()) {
    check_vec(*shift, a.C, "shift");
    TORCH_CHECK(shift->device() == x.device(), "shift must be on the device of the other operands");
    check_aligned16(*shift, "shift");
    psh = shift->data_ptr<float>();
  }
  TORCH_CHECK((int64_t)a.N * a.Ho * a.Wo * a.C < (1ll << 31), "dwconvk: y must have fewer than 2^31 "
              "elements");
  c10::DeviceGuard g(x.device());
  auto y = torch::empty({a.N, a.Ho, a.Wo, a.C}, x.options());
  optional<Tensor> ps, pss;
  Tensor ws;
  if (psh != nullptr) {
    auto o = x.options().dtype(at::kFloat);
    auto st = torch::empty({2, 1, a.C}, o);
    ps = st[0];
    pss = st[1];
    ws = torch::empty({2, (int64_t)mipipe::dwk_stat_rows(a.N, a.Ho, a.Wo, a.k, a.s), a.C}, o);
  }
  mipipe::dwconvk_fwd(x.data_ptr(), w.data_ptr(), psh, y.data_ptr(), wsp(ws),
                      psh ? ps->data_ptr<float>() : nullptr, psh ? pss->data_ptr<float>() : nullptr,
                      a.N, a.H, a.W, a.C, a.k, a.s, is_f32(x), stream());
  return {y, ps, pss};
}

// dx [N, H, W, C] = T(data-grad(dy) + addend); x_shape: the forward input's shape
Tensor dwconvk_dgrad(Tensor dy, Tensor w, std::vector<int64_t> x_shape, int64_t stride,
                     optional<Tensor> addend) {
  check_nhwc(dy, "dy");
  const int64_t k = check_weight(w, dy);
  check_ks(k, stride);
  TORCH_CHECK(x_shape.size() == 4 && x_shape[0] == dy.size(0) && x_shape[3] == dy.size(3) &&
                  x_shape[1] >= 1 && x_shape[2] >= 1,
              "x_shape must be [N, H, W, C] of the forward input");
  TORCH_CHECK(x_shape[0] * x_shape[1] * x_shape[2] * x_shape[3] < (1ll << 31),
              "dwconvk: dx must have fewer than 2^31 elements");
  DwkArgs a{(int)x_shape[0], (int)x_shape[1], (int)x_shape[2], (int)x_shape[3], 0, 0, (int)k,
            (int)stride};
  a.Ho = mipipe::dwk_out(a.H, a.k, a.s);
  a.Wo = mipipe::dwk_out(a.W, a.k, a.s);
  check_dy(dy, dy, a);
  c10::DeviceGuard g(dy.device());
  auto dx = torch::empty({a.N, a.H, a.W, a.C}, dy.options());
  if (addend.has_value()) {
    check_same(*addend, dy, "addend");
    TORCH_CHECK(addend->sizes() == dx.sizes(), "addend must have dx's shape ", dx.sizes(),
                ", got ", addend->sizes());
    TORCH_CHECK(addend->device() == dy.device(), "addend must be on the device of the other "
                "operands");
    check_aligned16(*addend, "addend");
  }
  mipipe::dwconvk_dgrad(dy.data_ptr(), w.data_ptr(), ptr_or_null(addend), dx.data_ptr(), a.N, a.H,
                        a.W, a.C, a.k, a.s, is_f32(dy), stream());
  return dx;
}

// dw [C, 1, K, K] fp32 += sum dy * x(shifted): ACCUMULATED into dw_acc (C*K*K floats, e.g. the
// flat-gradient view; returned as None) or into a new zeroed tensor
optional<Tensor> dwconvk_wgrad(Tensor dy, Tensor x, int64_t k, int64_t stride,
                               optional<Tensor> dw_acc) {
  const DwkArgs a = dwk_args(x, k, stride);
  check_dy(dy, x, a);
  c10::DeviceGuard g(x.device());
  auto o = x.options().dtype(at::kFloat);
  optional<Tensor> dw;
  float* pw = nullptr;
  if (dw_acc.has_value()) {
    check_vec(*dw_acc, (int64_t)a.C * k * k, "dw");
    TORCH_CHECK(dw_acc->device() == x.device(), "dw must be on the device of the other operands");
    pw = dw_acc->data_ptr<float>();
  } else {
    dw = torch::zeros({a.C, 1, k, k}, o);
    pw = dw->data_ptr<float>();
  }
  const int64_t P = mipipe::dwk_wgrad_rows(a.N, a.Ho, a.Wo, a.C, a.k, a.s, is_f32(x));
  auto ws = torch::empty({P, (int64_t)a.C * k * k}, o);
  mipipe::dwconvk_wgrad(dy.data_ptr(), x.data_ptr(), ws.data_ptr<float>(), pw, a.N, a.H, a.W, a.C,
                        a.k, a.s, is_f32(x), stream());
  return dw;
}

int64_t tile_h(int64_t k, int64_t s) {
  check_ks(k, s);
  return mipipe::dwk_tile_h((int)k, (int)s);
}
int64_t tile_w(int64_t k, int64_t s) {
  check_ks(k, s);
  return mipipe::dwk_tile_w((int)k, (int)s);
}
int64_t stat_rows(int64_t N, int64_t Ho, int64_t Wo, int64_t k, int64_t s) {
  check_ks(k, s);
  return mipipe::dwk_stat_rows((int)N, (int)Ho, (int)Wo, (int)k, (int)s);
}
int64_t wgrad_rows(int64_t N, int64_t Ho, int64_t Wo, int64_t C, int64_t k, int64_t s, bool f32) {
  check_ks(k, s);
  return mipipe::dwk_wgrad_rows((int)N, (int)Ho, (int)Wo, (int)C, (int)k, (int)s, f32);
}
int64_t lds_bytes(const std::string& pass, int64_t k, int64_t s) {
  check_ks(k, s);
  const int p = pass == "fwd" ? 0 : pass == "dgrad" ? 1 : pass == "wgrad" ? 2 : -1;
  TORCH_CHECK(p >= 0, "dwk_lds_bytes: pass must be fwd, dgrad or wgrad, got ", pass);
  return mipipe::dwk_lds_bytes(p, (int)k, (int)s);
}

}  // namespace

void bind_dwconvk(py::module& m) {
  m.def("dwconvk_fwd", &dwconvk_fwd, py::arg("x"), py::arg("w"), py::arg("stride"),
        py::arg("shift") = py::none());
  m.def("dwconvk_dgrad", &dwconvk_dgrad, py::arg("dy"), py::arg("w"), py::arg("x_shape"),
        py::arg("stride"), py::arg("addend") = py::none());
  m.def("dwconvk_wgrad", &dwconvk_wgrad, py::arg("dy"), py::arg("x"), py::arg("k"),
        py::arg("stride"), py::arg("dw") = py::none());
  m.def("dwk_tile_h", &tile_h, py::arg("k"), py::arg("stride"));
  m.def("dwk_tile_w", &tile_w, py::arg("k"), py::arg("stride"));
  m.def("dwk_stat_rows", &stat_rows, py::arg("N"), py::arg("Ho"), py::arg("Wo"), py::arg("k"),
        py::arg("stride"));
  m.def("dwk_wgrad_rows", &wgrad_rows, py::arg("N"), py::arg("Ho"), py::arg("Wo"), py::arg("C"),
        py::arg("k"), py::arg("stride"), py::arg("f32") = false);
  m.def("dwk_lds_bytes", &lds_bytes, py::arg("which"), py::arg("k"), py::arg("stride"));
  m.attr("DWK_CHAN_BLOCK") = mipipe::dwk_chan_block(false);
  m.attr("DWK_CHAN_BLOCK_F32") = mipipe::dwk_chan_block(true);
  m.attr("DWK_MAX_BLOCKS") = mipipe::kDwkMaxBlocks;
  m.attr("DWK_DGRAD_TILE") = mipipe::kDwkDgradTile;
  m.attr("DWK_WGRAD_BLOCKS") = mipipe::kDwkWgradBlocks;
  m.attr("DWK_WGRAD_MIN_ROWS") = mipipe::kDwkWgradMinRows;
  m.attr("DWK_WGRAD_MAX_ROWS") = mipipe::kDwkWgradMaxRows;
}

}  // namespace mipipe_bind
