// MaxViT entries of mipipe._C (kernels/relattn.hip): block / grid partition attention with a
// relative-position table, forward and backward.
#include "bind/common.hpp"

namespace mipipe_bind {
namespace {

bool grid_mode(const std::string& mode) {
  TORCH_CHECK(mode == "block" || mode == "grid",
              "partition_attention: mode must be \"block\" or \"grid\", got \"", mode, "\"");
  return mode == "grid";
}

// t [B*Hs*Ws, mult*heads*32] bf16, 16-byte aligned; 7x7 partitions
void check_tokens(const Tensor& t, const char* name, int64_t B, int64_t Hs, int64_t Ws,
                  int64_t heads, int64_t mult) {
  check_bf16(t, name);
  TORCH_CHECK(B >= 1 && heads >= 1 && Hs >= 1 && Ws >= 1 && t.numel() > 0,
              "partition_attention: empty input");
  TORCH_CHECK(Hs % 7 == 0 && Ws % 7 == 0, "partition_attention: the map ", Hs, "x", Ws,
              " is not a whole number of 7x7 partitions");
  TORCH_CHECK(B * Hs * Ws * 3 * heads * 32 < (1ll << 31),
              "partition_attention: qkv must have fewer than 2^31 elements");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == B * Hs * Ws && t.size(1) == mult * heads * 32, name,
              " must be [", B * Hs * Ws, ", ", mult * heads * 32, "] (head width 32), got ",
              t.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16-byte boundary");
}

const float* check_table(const Tensor& table, const Tensor& like, int64_t heads) {
  check_f32(table, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(0) == 169 && table.size(1) == heads,
              "table must be [169, ", heads, "], got ", table.sizes());
  TORCH_CHECK(table.device() == like.device(), "table must be on qkv's device");
  return table.data_ptr<float>();
}

Tensor relattn_fwd(Tensor qkv, Tensor table, int64_t B, int64_t Hs, int64_t Ws, int64_t heads,
                   std::string mode, double scale) {
  const bool grid = grid_mode(mode);
  check_tokens(qkv, "qkv", B, Hs, Ws, heads, 3);
  const float* tp = check_table(table, qkv, heads);
  c10::DeviceGuard g(qkv.device());
  auto o = torch::empty({qkv.size(0), heads * 32}, qkv.options());
  mipipe::relattn_fwd(qkv.data_ptr(), tp, o.data_ptr(), (int)B, (int)Hs, (int)Ws, (int)heads,
                      grid, (float)scale, stream());
  return o;
}

// -> (dqkv, dtable); the table gradient is ACCUMULATED into dtable_acc (fp32 [169*heads], e.g.
// the flat-gradient view) and returned as None, or into a new zeroed buffer when none is given
std::tuple<Tensor, optional<Tensor>> relattn_bwd(Tensor dout, Tensor qkv, Tensor table, int64_t B,
                                                 int64_t Hs, int64_t Ws, int64_t heads,
                                                 std::string mode, double scale,
                                                 optional<Tensor> dtable_acc) {
  const bool grid = grid_mode(mode);
  check_tokens(qkv, "qkv", B, Hs, Ws, heads, 3);
  check_tokens(dout, "dout", B, Hs, Ws, heads, 1);
  TORCH_CHECK(dout.device() == qkv.device(), "dout must be on qkv's device");
  const float* tp = check_table(table, qkv, heads);
  c10::DeviceGuard g(qkv.device());
  optional<Tensor> dtable;
  float* dt;
  if (dtable_acc.has_value()) {
    TORCH_CHECK(dtable_acc->device() == qkv.device(), "the accumulator must be on qkv's device");
    dt = fptr(dtable_acc, 169 * heads);
  } else {
    dtable = torch::zeros({169, heads}, qkv.options().dtype(at::kFloat));
    dt = dtable->data_ptr<float>();
  }
  auto dqkv = torch::empty_like(qkv);
  auto partial = torch::empty({(int64_t)mipipe::winattn_runs(B * (Hs / 7) * (Ws / 7)),
                               169 * heads}, qkv.options().dtype(at::kFloat));
  mipipe::relattn_bwd(dout.data_ptr(), qkv.data_ptr(), tp, dqkv.data_ptr(),
                      partial.data_ptr<float>(), dt, (int)B, (int)Hs, (int)Ws, (int)heads, grid,
                      (float)scale, stream());
  return {dqkv, dtable};
}

}  // namespace

void bind_maxvit(py::module& m) {
  m.def("relattn_fwd", &relattn_fwd, py::arg("qkv"), py::arg("table"), py::arg("batch"),
        py::arg("hs"), py::arg("ws"), py::arg("heads"), py::arg("mode"), py::arg("scale"));
  m.def("relattn_bwd", &relattn_bwd, py::arg("dout"), py::arg("qkv"), py::arg("table"),
        py::arg("batch"), py::arg("hs"), py::arg("ws"), py::arg("heads"), py::arg("mode"),
        py::arg("scale"), py::arg("dtable") = py::none());
}

}  // namespace mipipe_bind
