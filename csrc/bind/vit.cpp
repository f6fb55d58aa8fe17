// Vision Transformer entries of mipipe._C (kernels/vit.hip): the image -> patch-row permutation
// and the token assembly (class token, position embedding) with its batch-reducing backward.
#include "bind/common.hpp"

namespace mipipe_bind {
namespace {

inline void check_aligned16(const Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

// x [B, C, H, W] fp32 / bf16 (NCHW contiguous) -> [B*(H/P)*(W/P), C*P*P] bf16 / fp32
Tensor patchify(Tensor x, int64_t P, at::ScalarType dt) {
  check_act(x, "x");
  TORCH_CHECK(x.dim() == 4, "x must be [B, C, H, W], got ", x.dim(), " dimensions");
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(P == 4 || (P >= 8 && P % 8 == 0),
              "patch size must be 4 or a positive multiple of 8, got ", P);
  TORCH_CHECK(C >= 1, "x must have at least one channel");
  TORCH_CHECK(H >= P && W >= P && H % P == 0 && W % P == 0, "image ", H, "x", W,
              " is not a whole number of ", P, "x", P, " patches");
  TORCH_CHECK(x.numel() < (1ll << 31), "patchify: x must have fewer than 2^31 elements");
  TORCH_CHECK(dt == at::kBFloat16 || dt == at::kFloat, "dtype must be bfloat16 or float32");
  check_aligned16(x, "x");
  c10::DeviceGuard g(x.device());
  auto out = torch::empty({B * (H / P) * (W / P), C * P * P}, x.options().dtype(dt));
  mipipe::patchify(x.data_ptr(), out.data_ptr(), (int)B, (int)C, (int)H, (int)W, (int)P,
                   is_f32(x), dt == at::kFloat, stream());
  return out;
}

struct TokArgs {
  int64_t B, N, D;
};
// rows [B*(N + off), D] of an activation tensor against the position table's N + 1 rows
TokArgs tok_args(const Tensor& t, int64_t D, int64_t S, int64_t off, const char* name) {
  check_act(t, name);
  TORCH_CHECK(D >= 8 && D % 8 == 0, "the hidden size must be a positive multiple of 8, got ", D);
  TORCH_CHECK(S >= 2, "the position table must hold the class token and at least one patch");
  const int64_t N = S - 1;
  TORCH_CHECK(t.dim() == 2 && t.size(1) == D && t.size(0) >= 1 && t.size(0) % (N + off) == 0,
              name, " must be [B*", N + off, ", ", D, "], got [", t.size(0), ", ",
              t.dim() == 2 ? t.size(1) : -1, "]");
  TORCH_CHECK(t.numel() / N * S < (1ll << 31), "token tensor too large");
  check_aligned16(t, name);
  return {t.size(0) / (N + off), N, D};
}

// e [B*N, D], cls fp32 [D], pos fp32 [(N+1)*D] -> h [B*(N+1), D]
Tensor tokens_assemble_fwd(Tensor e, Tensor cls, Tensor pos) {
  check_f32(cls, "cls");
  check_f32(pos, "pos");
  const int64_t D = cls.numel();
  TORCH_CHECK(D > 0 && pos.numel() % D == 0, "pos must hold whole rows of cls's width");
  const TokArgs a = tok_args(e, D, pos.numel() / D, 0, "e");
  TORCH_CHECK(cls.device() == e.device() && pos.device() == e.device(),
              "cls and pos must be on e's device");
  check_aligned16(cls, "cls");
  check_aligned16(pos, "pos");
  c10::DeviceGuard g(e.device());
  auto h = torch::empty({a.B * (a.N + 1), D}, e.options());
  mipipe::tokens_assemble_fwd(e.data_ptr(), cls.data_ptr<float>(), pos.data_ptr<float>(),
                              h.data_ptr(), (int)a.B, (int)a.N, (int)D, is_f32(e), stream());
  return h;
}

// dh [B*(N+1), D] -> (de [B*N, D], dpos, dcls); the two sums are ACCUMULATED into dpos_acc
// [(N+1)*D] / dcls_acc [D] (fp32, e.g. the flat-gradient views) and returned as None, or into
// new zeroed buffers when none is given
std::tuple<Tensor, optional<Tensor>, optional<Tensor>> tokens_assemble_bwd(
    Tensor dh, int64_t batch, optional<Tensor> dpos_acc, optional<Tensor> dcls_acc) {
  TORCH_CHECK(dpos_acc.has_value() == dcls_acc.has_value(), "pass both accumulators or none");
  TORCH_CHECK(dh.dim() == 2 && batch >= 1 && dh.size(0) % batch == 0,
              "dh must be [batch*(N+1), D]");
  const int64_t D = dh.size(1), S = dh.size(0) / batch;
  const TokArgs a = tok_args(dh, D, S, 1, "dh");
  c10::DeviceGuard g(dh.device());
  auto o = dh.options().dtype(at::kFloat);
  optional<Tensor> dpos, dcls;
  float *pp, *pc;
  if (dpos_acc.has_value()) {
    pp = fptr(dpos_acc, S * D);
    pc = fptr(dcls_acc, D);
    TORCH_CHECK(dpos_acc->device() == dh.device() && dcls_acc->device() == dh.device(),
                "the accumulators must be on dh's device");
    check_aligned16(*dpos_acc, "dpos");
    check_aligned16(*dcls_acc, "dcls");
  } else {
    dpos = torch::zeros({S * D}, o);
    dcls = torch::zeros({D}, o);
    pp = dpos->data_ptr<float>();
    pc = dcls->data_ptr<float>();
  }
  auto de = torch::empty({a.B * a.N, D}, dh.options());
  mipipe::tokens_assemble_bwd(dh.data_ptr(), de.data_ptr(), pp, pc, (int)a.B, (int)a.N, (int)D,
                              is_f32(dh), stream());
  return {de, dpos, dcls};
}

}  // namespace

void bind_vit(py::module& m) {
  m.def("patchify", &patchify, py::arg("x"), py::arg("patch"), py::arg("dtype"));
  m.def("tokens_assemble_fwd", &tokens_assemble_fwd, py::arg("e"), py::arg("cls"),
        py::arg("pos"));
  m.def("tokens_assemble_bwd", &tokens_assemble_bwd, py::arg("dh"), py::arg("batch"),
        py::arg("dpos") = py::none(), py::arg("dcls") = py::none());
}

}  // namespace mipipe_bind
