// Grouped 3 x 3 entries of mipipe._C (kernels/gconv3.hip): group width G = C / groups with
// G % 8 == 0 and 8 <= G <= 64, pad 1, stride in {1, 2}, NHWC bf16, no bias: forward with
// BatchNorm's shifted statistics in the same pass, data-grad with an optional addend,
// atomics-free weight-grad.
#include "bind/common.hpp"

namespace mipipe_bind {
namespace {

inline void check_aligned16(const Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

struct Gc3Args {
  int N, H, W, C, G, Ho, Wo, s;
};
void check_stride(int64_t s) {
  TORCH_CHECK(s == 1 || s == 2, "gconv3: the stride must be 1 or 2, got ", s);
}
void check_width(int64_t C, int64_t G) {
  TORCH_CHECK(G >= 8 && G <= 64 && G % 8 == 0,
              "gconv3 needs a group width G with G % 8 == 0 and 8 <= G <= 64, got ", G);
  TORCH_CHECK(C % G == 0, "gconv3: C = ", C, " is no multiple of the group width ", G);
}
// t [N, h, w, C] NHWC bf16, non-empty, < 2^31 elements, 16-byte aligned
void check_nhwc(const Tensor& t, const char* name) {
  check_bf16(t, name);
  TORCH_CHECK(t.dim() == 4, name, " must be [N, H, W, C], got ", t.dim(), " dimensions");
  TORCH_CHECK(t.numel() > 0, name, " must not be empty");
  TORCH_CHECK(t.numel() < (1ll << 31), "gconv3: ", name, " must have fewer than 2^31 elements");
  check_aligned16(t, name);
}
// the operand weight [C, 3, 3, G] bf16 on ref's device; -> G
int64_t check_weight(const Tensor& w, const Tensor& ref) {
  check_bf16(w, "w");
  const int64_t C = ref.size(3);
  TORCH_CHECK(w.dim() == 4 && w.size(0) == C && w.size(1) == 3 && w.size(2) == 3,
              "w must be [", C, ", 3, 3, G], got ", w.sizes());
  check_width(C, w.size(3));
  TORCH_CHECK(w.device() == ref.device(), "w must be on the device of the other operands");
  check_aligned16(w, "w");
  return w.size(3);
}
Gc3Args gc3_args(int64_t N, int64_t H, int64_t W, int64_t C, int64_t G, int64_t s) {
  check_stride(s);
  check_width(C, G);
  Gc3Args a{(int)N, (int)H, (int)W, (int)C, (int)G, 0, 0, (int)s};
  a.Ho = mipipe::gc3_out(a.H, a.s);
  a.Wo = mipipe::gc3_out(a.W, a.s);
  return a;
}
void check_dy(const Tensor& dy, const Tensor& ref, const Gc3Args& a) {
  check_nhwc(dy, "dy");
  TORCH_CHECK(dy.size(0) == a.N && dy.size(1) == a.Ho && dy.size(2) == a.Wo && dy.size(3) == a.C,
              "dy must be [", a.N, ", ", a.Ho, ", ", a.Wo, ", ", a.C, "], got ", dy.sizes());
  TORCH_CHECK(dy.device() == ref.device(), "dy must be on the device of the other operands");
}

// -> (y, ps, pss): y = bf16(conv(x, w)); with shift (fp32 [C]) also ps / pss [1, C] fp32, the sums
// of (y - shift) and its square over the STORED y, else None
std::tuple<Tensor, optional<Tensor>, optional<Tensor>> gconv3_fwd(Tensor x, Tensor w, int64_t stride,
                                                                  optional<Tensor> shift) {
  check_nhwc(x, "x");
  const Gc3Args a = gc3_args(x.size(0), x.size(1), x.size(2), x.size(3), check_weight(w, x), stride);
  const float* psh = nullptr;
  if (shift.has_value()) {
    check_vec(*shift, a.C, "shift");
    TORCH_CHECK(shift->device() == x.device(), "shift must be on the device of the other operands");
    check_aligned16(*shift, "shift");
    psh = shift->data_ptr<float>();
  }
  c10::DeviceGuard g(x.device());
  auto y = torch::empty({a.N, a.Ho, a.Wo, a.C}, x.options());
  optional<Tensor> ps, pss;
  Tensor ws;
  if (psh != nullptr) {
    auto o = x.options().dtype(at::kFloat);
    auto st = torch::empty({2, 1, a.C}, o);
    ps = st[0];
    pss = st[1];
    ws = torch::empty({2, (int64_t)mipipe::gc3_stat_rows(a.N, a.Ho, a.Wo, a.s), a.C}, o);
  }
  mipipe::gconv3_fwd(x.data_ptr(), w.data_ptr(), psh, y.data_ptr(), wsp(ws),
                     psh ? ps->data_ptr<float>() : nullptr, psh ? pss->data_ptr<float>() : nullptr,
                     a.N, a.H, a.W, a.C, a.G, a.s, stream());
  return {y, ps, pss};
}

// dx [N, H, W, C] = bf16(data-grad(dy) + addend); x_shape: the forward input's shape
Tensor gconv3_dgrad(Tensor dy, Tensor w, std::vector<int64_t> x_shape, int64_t stride,
                    optional<Tensor> addend) {
  check_nhwc(dy, "dy");
  const int64_t G = check_weight(w, dy);
  TORCH_CHECK(x_shape.size() == 4 && x_shape[0] == dy.size(0) && x_shape[3] == dy.size(3) &&
                  x_shape[1] >= 1 && x_shape[2] >= 1,
              "x_shape must be [N, H, W, C] of the forward input");
  TORCH_CHECK(x_shape[0] * x_shape[1] * x_shape[2] * x_shape[3] < (1ll << 31),
              "gconv3: dx must have fewer than 2^31 elements");
  const Gc3Args a = gc3_args(x_shape[0], x_shape[1], x_shape[2], x_shape[3], G, stride);
  check_dy(dy, dy, a);
  c10::DeviceGuard g(dy.device());
  auto dx = torch::empty({a.N, a.H, a.W, a.C}, dy.options());
  if (addend.has_value()) {
    check_bf16(*addend, "addend");
    TORCH_CHECK(addend->sizes() == dx.sizes(), "addend must have dx's shape ", dx.sizes(),
                ", got ", addend->sizes());
    TORCH_CHECK(addend->device() == dy.device(), "addend must be on the device of the other "
                "operands");
    check_aligned16(*addend, "addend");
  }
  mipipe::gconv3_dgrad(dy.data_ptr(), w.data_ptr(), ptr_or_null(addend), dx.data_ptr(), a.N, a.H,
                       a.W, a.C, a.G, a.s, stream());
  return dx;
}

// dw [C, G, 3, 3] fp32 += sum dy * x(shifted): ACCUMULATED into dw_acc (returned as None) or into
// a new zeroed tensor.  dw_acc: C*G*9 floats in [C, G, 3, 3] order, or a [C, G, 3, 3] tensor that
// is contiguous or channels-last (the parameter's flat-gradient view: stored as [C, 3, 3, G])
optional<Tensor> gconv3_wgrad(Tensor dy, Tensor x, int64_t G, int64_t stride,
                              optional<Tensor> dw_acc) {
  check_nhwc(x, "x");
  const Gc3Args a = gc3_args(x.size(0), x.size(1), x.size(2), x.size(3), G, stride);
  check_dy(dy, x, a);
  c10::DeviceGuard g(x.device());
  auto o = x.options().dtype(at::kFloat);
  optional<Tensor> dw;
  float* pw = nullptr;
  bool chl = false;
  if (dw_acc.has_value()) {
    const Tensor& t = *dw_acc;
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.device() == x.device(),
                "dw must be float32 on the device of the other operands");
    TORCH_CHECK(t.numel() == (int64_t)a.C * G * 9, "dw must have ", (int64_t)a.C * G * 9,
                " elements, got ", t.numel());
    const bool shaped = t.dim() == 4 && t.size(0) == a.C && t.size(1) == G && t.size(2) == 3;
    chl = shaped && !t.is_contiguous() && t.is_contiguous(at::MemoryFormat::ChannelsLast);
    TORCH_CHECK(chl || (t.is_contiguous() && (shaped || t.dim() == 1)),
                "dw must be [C*G*9] or [C, G, 3, 3], contiguous or channels-last");
    pw = t.data_ptr<float>();
  } else {
    dw = torch::zeros({a.C, G, 3, 3}, o);
    pw = dw->data_ptr<float>();
  }
  const int64_t P = mipipe::gc3_wgrad_rows(a.N, a.Ho, a.Wo, a.C, a.G, a.s);
  auto ws = torch::empty({P, (int64_t)a.C * G * 9}, o);
  mipipe::gconv3_wgrad(dy.data_ptr(), x.data_ptr(), ws.data_ptr<float>(), pw, a.N, a.H, a.W, a.C,
                       a.G, a.s, chl, stream());
  return dw;
}

int64_t tile_h(int64_t s) {
  check_stride(s);
  return mipipe::gc3_tile_h((int)s);
}
int64_t tile_w(int64_t s) {
  check_stride(s);
  return mipipe::gc3_tile_w((int)s);
}
int64_t groups_per_block(int64_t G) {
  check_width(G, G);
  return mipipe::gc3_groups_per_block((int)G);
}
int64_t stat_rows(int64_t N, int64_t Ho, int64_t Wo, int64_t s) {
  check_stride(s);
  return mipipe::gc3_stat_rows((int)N, (int)Ho, (int)Wo, (int)s);
}
int64_t wgrad_rows(int64_t N, int64_t Ho, int64_t Wo, int64_t C, int64_t G, int64_t s) {
  check_stride(s);
  check_width(C, G);
  return mipipe::gc3_wgrad_rows((int)N, (int)Ho, (int)Wo, (int)C, (int)G, (int)s);
}

}  // namespace

void bind_gconv3(py::module& m) {
  m.def("gconv3_fwd", &gconv3_fwd, py::arg("x"), py::arg("w"), py::arg("stride"),
        py::arg("shift") = py::none());
  m.def("gconv3_dgrad", &gconv3_dgrad, py::arg("dy"), py::arg("w"), py::arg("x_shape"),
        py::arg("stride"), py::arg("addend") = py::none());
  m.def("gconv3_wgrad", &gconv3_wgrad, py::arg("dy"), py::arg("x"), py::arg("G"),
        py::arg("stride"), py::arg("dw") = py::none());
  m.def("gc3_tile_h", &tile_h, py::arg("stride"));
  m.def("gc3_tile_w", &tile_w, py::arg("stride"));
  m.def("gc3_groups_per_block", &groups_per_block, py::arg("G"));
  m.def("gc3_stat_rows", &stat_rows, py::arg("N"), py::arg("Ho"), py::arg("Wo"), py::arg("stride"));
  m.def("gc3_wgrad_rows", &wgrad_rows, py::arg("N"), py::arg("Ho"), py::arg("Wo"), py::arg("C"),
        py::arg("G"), py::arg("stride"));
  m.attr("GC3_MAX_BLOCKS") = mipipe::kGc3MaxBlocks;
  m.attr("GC3_DGRAD_TILE") = mipipe::kGc3DgradTile;
  m.attr("GC3_WGRAD_MAX_ROWS") = mipipe::kGc3WgradMaxRows;
}

}  // namespace mipipe_bind
