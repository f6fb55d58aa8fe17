// Swin Transformer entries of mipipe._C (kernels/winattn.hip, winattn8.hip): shifted-window
// attention forward and backward (V1: 7x7 windows, V2: 8x8 windows with cosine scores), and the
// PatchMerging permutation with its inverse.
#include "bind/common.hpp"

namespace mipipe_bind {
namespace {

inline void check_aligned16(const Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

// t [B*Hs*Ws, mult*heads*32] bf16 of a window-attention call with win x win windows (op names it)
void check_win(int64_t win, const char* op, const Tensor& t, const char* name, int64_t B,
               int64_t Hs, int64_t Ws, int64_t heads, int64_t mult, int64_t sy, int64_t sx) {
  const int64_t shift = win / 2;
  check_bf16(t, name);
  TORCH_CHECK(B >= 1 && heads >= 1 && Hs >= 1 && Ws >= 1 && t.numel() > 0, op, ": empty input");
  TORCH_CHECK(Hs % win == 0 && Ws % win == 0, op, ": the map ", Hs, "x", Ws,
              " is not a whole number of ", win, "x", win, " windows");
  TORCH_CHECK((sy == 0 || sy == shift) && (sx == 0 || sx == shift), op,
              ": the shift must be 0 or ", shift, " per axis, got (", sy, ", ", sx, ")");
  TORCH_CHECK(B * Hs * Ws * 3 * heads * 32 < (1ll << 31), op,
              ": qkv must have fewer than 2^31 elements");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == B * Hs * Ws && t.size(1) == mult * heads * 32, name,
              " must be [", B * Hs * Ws, ", ", mult * heads * 32, "] (head width 32), got ",
              t.sizes());
  check_aligned16(t, name);
}

// where a parameter gradient is accumulated: acc (fp32, n elements, e.g. a flat-gradient view),
// or a new zeroed buffer of the given shape, left in fresh, when no accumulator is given
float* grad_target(const optional<Tensor>& acc, optional<Tensor>& fresh, at::IntArrayRef shape,
                   int64_t n, const Tensor& like) {
  if (acc.has_value()) {
    TORCH_CHECK(acc->device() == like.device(), "the accumulator must be on qkv's device");
    return fptr(acc, n);
  }
  fresh = torch::zeros(shape, like.options().dtype(at::kFloat));
  return fresh->data_ptr<float>();
}

const float* check_table(const Tensor& table, const Tensor& like, int64_t heads) {
  check_vec(table, 169 * heads, "table");
  TORCH_CHECK(table.device() == like.device(), "table must be on qkv's device");
  return table.data_ptr<float>();
}

Tensor winattn_fwd(Tensor qkv, Tensor table, int64_t B, int64_t Hs, int64_t Ws, int64_t heads,
                   int64_t sy, int64_t sx) {
  check_win(7, "window_attention", qkv, "qkv", B, Hs, Ws, heads, 3, sy, sx);
  const float* tp = check_table(table, qkv, heads);
  c10::DeviceGuard g(qkv.device());
  auto o = torch::empty({qkv.size(0), heads * 32}, qkv.options());
  mipipe::winattn_fwd(qkv.data_ptr(), tp, o.data_ptr(), (int)B, (int)Hs, (int)Ws, (int)heads,
                      (int)sy, (int)sx, stream());
  return o;
}

// -> (dqkv, dtable); the table gradient is ACCUMULATED into dtable_acc (fp32 [169*heads], e.g.
// the flat-gradient view) and returned as None, or into a new zeroed buffer when none is given
std::tuple<Tensor, optional<Tensor>> winattn_bwd(Tensor dout, Tensor qkv, Tensor table, int64_t B,
                                                 int64_t Hs, int64_t Ws, int64_t heads, int64_t sy,
                                                 int64_t sx, optional<Tensor> dtable_acc) {
  check_win(7, "window_attention", qkv, "qkv", B, Hs, Ws, heads, 3, sy, sx);
  check_win(7, "window_attention", dout, "dout", B, Hs, Ws, heads, 1, sy, sx);
  TORCH_CHECK(dout.device() == qkv.device(), "dout must be on qkv's device");
  const float* tp = check_table(table, qkv, heads);
  c10::DeviceGuard g(qkv.device());
  optional<Tensor> dtable;
  float* dt = grad_target(dtable_acc, dtable, {169, heads}, 169 * heads, qkv);
  auto dqkv = torch::empty_like(qkv);
  auto partial = torch::empty({(int64_t)mipipe::winattn_runs(B * (Hs / 7) * (Ws / 7)),
                               169 * heads}, qkv.options().dtype(at::kFloat));
  mipipe::winattn_bwd(dout.data_ptr(), qkv.data_ptr(), tp, dqkv.data_ptr(),
                      partial.data_ptr<float>(), dt, (int)B, (int)Hs, (int)Ws, (int)heads, (int)sy,
                      (int)sx, stream());
  return {dqkv, dtable};
}

// ---- Swin V2 (winattn8.hip): 8x8 windows, cosine scores
// bias fp32 [225, heads], logit_scale fp32 [heads] on qkv's device
void check_win8_params(const Tensor& bias, const Tensor& logit_scale, const Tensor& like,
                       int64_t heads) {
  check_f32(bias, "bias");
  check_f32(logit_scale, "logit_scale");
  TORCH_CHECK(bias.dim() == 2 && bias.size(0) == 225 && bias.size(1) == heads,
              "bias must be [225, ", heads, "], got ", bias.sizes());
  TORCH_CHECK(logit_scale.dim() == 1 && logit_scale.size(0) == heads, "logit_scale must be [",
              heads, "], got ", logit_scale.sizes());
  TORCH_CHECK(bias.device() == like.device() && logit_scale.device() == like.device(),
              "bias and logit_scale must be on qkv's device");
}

Tensor winattn8_fwd(Tensor qkv, Tensor bias, Tensor logit_scale, int64_t B, int64_t Hs,
                    int64_t Ws, int64_t heads, int64_t sy, int64_t sx) {
  check_win(8, "window_attention_v2", qkv, "qkv", B, Hs, Ws, heads, 3, sy, sx);
  check_win8_params(bias, logit_scale, qkv, heads);
  c10::DeviceGuard g(qkv.device());
  auto o = torch::empty({qkv.size(0), heads * 32}, qkv.options());
  mipipe::winattn8_fwd(qkv.data_ptr(), bias.data_ptr<float>(), logit_scale.data_ptr<float>(),
                       o.data_ptr(), (int)B, (int)Hs, (int)Ws, (int)heads, (int)sy, (int)sx,
                       stream());
  return o;
}

// -> (dqkv, dbias, dlogit_scale); each of the two parameter gradients is ACCUMULATED into its
// accumulator (fp32 [225*heads] / [heads], e.g. a flat-gradient view) and returned as None, or
// into a new zeroed buffer when none is given
std::tuple<Tensor, optional<Tensor>, optional<Tensor>> winattn8_bwd(
    Tensor dout, Tensor qkv, Tensor bias, Tensor logit_scale, int64_t B, int64_t Hs, int64_t Ws,
    int64_t heads, int64_t sy, int64_t sx, optional<Tensor> dbias_acc,
    optional<Tensor> dlogit_acc) {
  check_win(8, "window_attention_v2", qkv, "qkv", B, Hs, Ws, heads, 3, sy, sx);
  check_win(8, "window_attention_v2", dout, "dout", B, Hs, Ws, heads, 1, sy, sx);
  TORCH_CHECK(dout.device() == qkv.device(), "dout must be on qkv's device");
  check_win8_params(bias, logit_scale, qkv, heads);
  c10::DeviceGuard g(qkv.device());
  optional<Tensor> dbias, dlogit;
  float* db = grad_target(dbias_acc, dbias, {225, heads}, 225 * heads, qkv);
  float* dl = grad_target(dlogit_acc, dlogit, {heads}, heads, qkv);
  auto dqkv = torch::empty_like(qkv);
  auto partial = torch::empty({(int64_t)mipipe::winattn_runs(B * (Hs / 8) * (Ws / 8)),
                               226 * heads}, qkv.options().dtype(at::kFloat));
  mipipe::winattn8_bwd(dout.data_ptr(), qkv.data_ptr(), bias.data_ptr<float>(),
                       logit_scale.data_ptr<float>(), dqkv.data_ptr(), partial.data_ptr<float>(),
                       db, dl, (int)B, (int)Hs, (int)Ws, (int)heads, (int)sy, (int)sx, stream());
  return {dqkv, dbias, dlogit};
}

// x [B*Hs*Ws, C] (or any shape with that many elements) -> [B*Hs/2*Ws/2, 4C]; bwd: the inverse
Tensor patch_merge(Tensor t, int64_t B, int64_t Hs, int64_t Ws, bool bwd) {
  check_bf16(t, bwd ? "dy" : "x");
  TORCH_CHECK(B >= 1 && Hs >= 1 && Ws >= 1 && t.numel() > 0, "patch_merge: empty input");
  TORCH_CHECK(Hs % 2 == 0 && Ws % 2 == 0, "patch_merge: the map ", Hs, "x", Ws,
              " must have even sides");
  TORCH_CHECK(t.numel() % (B * Hs * Ws) == 0, "patch_merge: ", t.numel(),
              " elements are not [", B, ", ", Hs, ", ", Ws, ", C]");
  const int64_t C = t.numel() / (B * Hs * Ws);
  TORCH_CHECK(C % 8 == 0, "patch_merge: C must be a multiple of 8, got ", C);
  TORCH_CHECK(t.numel() < (1ll << 31), "patch_merge: fewer than 2^31 elements are supported");
  check_aligned16(t, bwd ? "dy" : "x");
  c10::DeviceGuard g(t.device());
  auto out = bwd ? torch::empty({B * Hs * Ws, C}, t.options())
                 : torch::empty({B * (Hs / 2) * (Ws / 2), 4 * C}, t.options());
  mipipe::patch_merge(t.data_ptr(), out.data_ptr(), (int)B, (int)Hs, (int)Ws, (int)C, bwd,
                      stream());
  return out;
}

}  // namespace

void bind_swin(py::module& m) {
  m.def("winattn_fwd", &winattn_fwd, py::arg("qkv"), py::arg("table"), py::arg("batch"),
        py::arg("hs"), py::arg("ws"), py::arg("heads"), py::arg("shift_y"), py::arg("shift_x"));
  m.def("winattn_bwd", &winattn_bwd, py::arg("dout"), py::arg("qkv"), py::arg("table"),
        py::arg("batch"), py::arg("hs"), py::arg("ws"), py::arg("heads"), py::arg("shift_y"),
        py::arg("shift_x"), py::arg("dtable") = py::none());
  m.def("patch_merge", &patch_merge, py::arg("x"), py::arg("batch"), py::arg("hs"), py::arg("ws"),
        py::arg("bwd") = false);
  m.def("winattn8_fwd", &winattn8_fwd, py::arg("qkv"), py::arg("bias"), py::arg("logit_scale"),
        py::arg("batch"), py::arg("hs"), py::arg("ws"), py::arg("heads"), py::arg("shift_y"),
        py::arg("shift_x"));
  m.def("winattn8_bwd", &winattn8_bwd, py::arg("dout"), py::arg("qkv"), py::arg("bias"),
        py::arg("logit_scale"), py::arg("batch"), py::arg("hs"), py::arg("ws"), py::arg("heads"),
        py::arg("shift_y"), py::arg("shift_x"), py::arg("dbias") = py::none(),
        py::arg("dlogit_scale") = py::none());
  // launch geometry, for the tests' edge shapes (one set of constants serves both kernels)
  m.attr("WIN_WAVES") = mipipe::kWinWaves;
  m.attr("WIN_RUN") = mipipe::kWinRun;
  m.attr("WIN_MAX_RUNS") = mipipe::kWinMaxRuns;
  m.attr("WIN8_WAVES") = mipipe::kWinWaves;
  m.attr("WIN8_RUN") = mipipe::kWinRun;
  m.attr("WIN8_MAX_RUNS") = mipipe::kWinMaxRuns;
}

}  // namespace mipipe_bind
