// Input-pipeline entries of mipipe._C: layout conversion, synthetic data, the record loaders'
// decode / augment / erase kernels and Mixup / CutMix of a batch.
#include "bind/common.hpp"
#include "common/augment.hpp"

namespace mipipe_bind {
namespace {

Tensor nchw_to_nhwc(Tensor x, at::ScalarType dtype, int64_t pad_to) {
  check_cuda(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(dtype == at::kBFloat16 || dtype == at::kFloat, "nchw_to_nhwc produces bf16 / fp32");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "x must be fp32/bf16");
  TORCH_CHECK(x.dim() == 4, "x must be NCHW");
  int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  int Cp = C;
  if (pad_to > 0 && C % pad_to) Cp = (int)((C + pad_to - 1) / pad_to * pad_to);
  Cp = (Cp + 7) / 8 * 8;
  auto y = torch::empty({N, H, W, Cp}, x.options().dtype(dtype));
  mipipe::nchw_to_nhwc(x.data_ptr(), x.scalar_type() == at::kBFloat16, y.data_ptr(), N, C, H, W, Cp,
                       stream(), dtype == at::kFloat);
  return y;
}

std::tuple<Tensor, Tensor> synthetic_batch(Tensor idx, int C, int H, int W, int classes, int seed,
                                           at::ScalarType dtype) {
  check_cuda(idx, "indices");
  c10::DeviceGuard g(idx.device());
  TORCH_CHECK(idx.scalar_type() == at::kLong, "indices must be int64");
  int n = idx.numel();
  bool bf = dtype == at::kBFloat16;
  TORCH_CHECK(bf || dtype == at::kFloat, "synthetic dtype must be fp32 or bf16");
  auto x = torch::empty({n, C, H, W}, idx.options().dtype(dtype));
  auto lab = torch::empty({n}, idx.options().dtype(at::kLong));
  mipipe::synthetic_batch(idx.data_ptr<int64_t>(), n, C, H, W, classes, seed, x.data_ptr(), bf,
                          lab.data_ptr<int64_t>(), stream());
  return {x, lab};
}

// the per-channel (scale, offset) of the decode kernels: fp32 [2, C] on the records' device
void check_affine(const Tensor& affine, const Tensor& rec, int64_t C) {
  check_f32(affine, "affine");
  TORCH_CHECK(affine.device() == rec.device(), "affine must be on the records' device");
  TORCH_CHECK(affine.dim() == 2 && affine.size(0) == 2 && affine.size(1) == C,
              "affine must be [2, C]");
}

// The record loader's crop / flip / normalise on the device: rec [n, label_bytes + C*H*W] uint8
// whole records, idx [n] int64 sample indices, affine [2, C] fp32 -> (x [n,C,H,W], y [n] int64).
std::tuple<Tensor, Tensor> record_decode(Tensor rec, Tensor idx, Tensor affine, int64_t C,
                                         int64_t H, int64_t W, uint64_t seed, int64_t epoch,
                                         int64_t pad, bool flip, bool train, int64_t label_bytes,
                                         at::ScalarType dtype) {
  const bool bf = dtype == at::kBFloat16;
  TORCH_CHECK(bf || dtype == at::kFloat, "record_decode produces fp32 or bf16");
  TORCH_CHECK(C >= 1 && H >= 1 && W >= 1 && C * H * W < (1ll << 31), "bad image shape");
  TORCH_CHECK(pad >= 0 && pad < (1 << 20), "bad pad ", pad);
  const int64_t n = check_records(rec, idx, C, H, W, label_bytes);
  check_affine(affine, rec, C);
  c10::DeviceGuard g(rec.device());
  auto x = torch::empty({n, C, H, W}, rec.options().dtype(dtype));
  auto y = torch::empty({n}, rec.options().dtype(at::kLong));
  if (n == 0) return {x, y};
  mipipe::record_decode(rec.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(), affine.data_ptr<float>(),
                        x.data_ptr(), bf, y.data_ptr<int64_t>(), n, (int)C, (int)H, (int)W,
                        (int)label_bytes, seed, (uint64_t)epoch, (int)pad, flip, train, stream());
  return {x, y};
}

// The loader's "rrc" transform on the device (RandomResizedCrop / centre crop + bilinear resize
// + flip + normalise): same inputs as record_decode, x is [n, C, Ho, Wo].
std::tuple<Tensor, Tensor> record_decode_rrc(Tensor rec, Tensor idx, Tensor affine, int64_t C,
                                             int64_t H, int64_t W, int64_t Ho, int64_t Wo,
                                             uint64_t seed, int64_t epoch, bool flip, bool train,
                                             int64_t label_bytes, at::ScalarType dtype) {
  const bool bf = dtype == at::kBFloat16;
  TORCH_CHECK(bf || dtype == at::kFloat, "record_decode_rrc produces fp32 or bf16");
  TORCH_CHECK(C >= 1 && H >= 2 && W >= 2 && H <= 32768 && W <= 32768 &&
                  C * H * W < (1ll << 31), "bad stored shape (H, W in [2, 32768])");
  TORCH_CHECK(Ho >= 1 && Wo >= 1 && Ho + Wo <= mipipe::record_decode_rrc_max_extent_sum &&
                  C * Ho * Wo < (1ll << 31),
              "bad output size ", Ho, "x", Wo, " (positive, Ho + Wo <= ",
              mipipe::record_decode_rrc_max_extent_sum, ")");
  const int64_t n = check_records(rec, idx, C, H, W, label_bytes);
  check_affine(affine, rec, C);
  c10::DeviceGuard g(rec.device());
  auto x = torch::empty({n, C, Ho, Wo}, rec.options().dtype(dtype));
  auto y = torch::empty({n}, rec.options().dtype(at::kLong));
  if (n == 0) return {x, y};
  mipipe::record_decode_rrc(rec.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(),
                            affine.data_ptr<float>(), x.data_ptr(), bf, y.data_ptr<int64_t>(), n,
                            (int)C, (int)H, (int)W, (int)Ho, (int)Wo, (int)label_bytes, seed,
                            (uint64_t)epoch, flip, train, stream());
  return {x, y};
}

// TrivialAugmentWide of whole records on the device (augment.hip): rec [n, label_bytes + C*H*W]
// uint8, idx [n] int64 -> a new record tensor of the same layout, for the decode kernels to read.
// force < 0: the op is a hash of (seed, epoch, idx); else op | m << 8 | (sign is +) << 16.
Tensor record_augment(Tensor rec, Tensor idx, int64_t C, int64_t H, int64_t W, uint64_t seed,
                      int64_t epoch, int64_t label_bytes, int64_t force, int64_t parts) {
  TORCH_CHECK(C == 1 || C == 3, "record_augment needs 1 or 3 channels, got ", C);
  TORCH_CHECK(H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && C * H * W < (1ll << 31) - 16,
              "bad image shape (H, W in [1, 32768])");
  const int64_t n = check_records(rec, idx, C, H, W, label_bytes);
  c10::DeviceGuard g(rec.device());
  TORCH_CHECK(mipipe_aug::force_ok(force), "bad force word ", force,
              " (op | m << 8 | sign << 16, op < 14, m < 31)");
  TORCH_CHECK(parts >= 0 && parts <= 64, "parts must be in [0, 64] (0: chosen by size)");
  auto out = torch::empty_like(rec);
  if (n == 0) return out;
  mipipe::record_augment(rec.data_ptr<uint8_t>(), idx.data_ptr<int64_t>(), out.data_ptr<uint8_t>(),
                         n, (int)C, (int)H, (int)W, (int)label_bytes, seed, (uint64_t)epoch,
                         (long)force, (int)parts, stream());
  return out;
}

// Random Erasing in place on the decoded batch x [n, C, Ho, Wo] (fp32 / bf16): the box of sample
// idx[s] (a hash of seed, epoch and idx[s]; applied with probability pq / 2^24) becomes 0.0.
Tensor batch_erase_(Tensor x, Tensor idx, uint64_t seed, int64_t epoch, int64_t pq) {
  check_act(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.dim() == 4, "x must be [n, C, Ho, Wo], got ", x.dim(), " dimensions");
  const int64_t n = x.size(0), C = x.size(1), Ho = x.size(2), Wo = x.size(3);
  TORCH_CHECK(Ho <= 32768 && Wo <= 32768 && C * Ho * Wo < (1ll << 31) - 4 * C * Ho,
              "sample too large (Ho, Wo <= 32768, C*Ho*Wo < 2^31)");
  check_sample_idx(idx, x, n);
  TORCH_CHECK(pq >= 0 && pq <= (1 << 24), "pq must be in [0, 2^24], got ", pq);
  if (x.numel() == 0 || pq == 0) return x;
  mipipe::batch_erase(x.data_ptr(), is_f32(x), idx.data_ptr<int64_t>(), n, (int)C, (int)Ho,
                      (int)Wo, seed, (uint64_t)epoch, (uint32_t)pq, stream());
  return x;
}

// Mixup / CutMix of x [B, C, H, W] with its reverse, as the device descriptor says (mix.hip).
// out: x itself (in place), another tensor of x's shape and type, or none (a new tensor).
Tensor batch_mix(Tensor x, Tensor mix, optional<Tensor> out) {
  check_act(x, "x");
  check_mix(mix, x);
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.dim() == 4, "x must be [B, C, H, W], got ", x.dim(), " dimensions");
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(B < (1ll << 31) && C * H * W < (1ll << 31), "sample too large: C*H*W must be < 2^31");
  Tensor o = out.has_value() ? *out : torch::empty_like(x);
  if (out.has_value()) {
    check_same(o, x, "out");
    TORCH_CHECK(o.sizes() == x.sizes() && o.device() == x.device(),
                "out must have x's shape and device");
    const char* xb = static_cast<const char*>(x.data_ptr());
    const char* ob = static_cast<const char*>(o.data_ptr());
    const int64_t nb = (int64_t)x.numel() * x.element_size();
    TORCH_CHECK(ob == xb || ob + nb <= xb || xb + nb <= ob, "out overlaps x without being x");
  }
  {
    const char* mb = static_cast<const char*>(mix.data_ptr());
    const char* ob = static_cast<const char*>(o.data_ptr());
    const int64_t nb = (int64_t)o.numel() * o.element_size();
    TORCH_CHECK(mb + mix.numel() * 4 <= ob || ob + nb <= mb, "mix overlaps out");
  }
  if (x.numel() == 0) return o;
  mipipe::batch_mix(x.data_ptr(), o.data_ptr(), mix.data_ptr<float>(), (int)B, (int)C, (int)H,
                    (int)W, is_f32(x), stream());
  return o;
}

}  // namespace

void bind_data(py::module& m) {
  m.def("nchw_to_nhwc", &nchw_to_nhwc);
  m.def("synthetic_batch", &synthetic_batch);
  m.def("record_decode", &record_decode, py::arg("rec"), py::arg("idx"), py::arg("affine"),
        py::arg("C"), py::arg("H"), py::arg("W"), py::arg("seed"), py::arg("epoch"),
        py::arg("pad"), py::arg("flip"), py::arg("train"), py::arg("label_bytes"),
        py::arg("dtype"));
  m.def("record_decode_rrc", &record_decode_rrc, py::arg("rec"), py::arg("idx"),
        py::arg("affine"), py::arg("C"), py::arg("H"), py::arg("W"), py::arg("Ho"), py::arg("Wo"),
        py::arg("seed"), py::arg("epoch"), py::arg("flip"), py::arg("train"),
        py::arg("label_bytes"), py::arg("dtype"));
  m.def("record_augment", &record_augment, py::arg("rec"), py::arg("idx"), py::arg("C"),
        py::arg("H"), py::arg("W"), py::arg("seed"), py::arg("epoch"), py::arg("label_bytes"),
        py::arg("force") = -1, py::arg("parts") = 0);
  m.def("record_augment_parts", &mipipe::record_augment_parts, py::arg("C"), py::arg("H"),
        py::arg("W"));
  m.def("batch_erase_", &batch_erase_, py::arg("x"), py::arg("idx"), py::arg("seed"),
        py::arg("epoch"), py::arg("pq"));
  m.def("batch_mix", &batch_mix, py::arg("x"), py::arg("mix"), py::arg("out") = py::none());
}

}  // namespace mipipe_bind
