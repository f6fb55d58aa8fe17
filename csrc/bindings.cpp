// Python bindings of mipipe's gfx950 kernels (module ``mipipe._C``).
//
// Every entry validates dtypes, contiguity and the shape constraints the kernels and their
// grids assume (NHWC, channels % 8 == 0, K % 8 == 0 ...) on the HOST before launching, so a bad
// call raises a Python error instead of faulting the GPU.  Outputs are allocated with the torch
// caching allocator and kernels run on the current HIP stream (graph-capturable).
#include <torch/extension.h>

#include <unordered_map>

#include "bind/common.hpp"

// the shared helpers and checks (stream, check_*, ce_args, check_records ...): bind/common.hpp
using namespace mipipe_bind;

namespace {

// bf16 operands go through buffer descriptors with 32-bit byte offsets (gemm_core.hpp kOOB,
// gk_rsrc clamps the range): a larger bf16 tensor would read zeros, so every conv entry point
// (forward, data-grad, weight-grad) checks its input and output sizes here.
void check_conv_buf_bytes(const mipipe::ConvShape& s, bool f32, const char* what) {
  if (f32) return;
  const int64_t lim = (1ll << 31) - (1ll << 24);
  TORCH_CHECK((int64_t)s.N * s.H * s.W * s.Ci * 2 < lim && (int64_t)s.N * s.Ho * s.Wo * s.Co * 2 < lim,
              "bf16 ", what, " tensors beyond 2 GiB are not supported");
}

// The one place a ConvShape is filled: sizes, strides / paddings in the struct's conventions
// (stride_w 0 = same as stride, pad_w -1 = same as pad) and the output extent.  The callers
// check what their kernels need.
mipipe::ConvShape make_conv_shape(int64_t N, int64_t H, int64_t W, int64_t Ci, int64_t Co, int KH,
                                  int KW, int stride, int pad, int stride_w, int pad_w, bool f32) {
  mipipe::ConvShape s;
  s.N = (int)N; s.H = (int)H; s.W = (int)W; s.Ci = (int)Ci;
  s.Co = (int)Co; s.KH = KH; s.KW = KW; s.stride = stride; s.pad = pad;
  s.stride_w = stride_w > 0 ? stride_w : 0;
  s.pad_w = pad_w >= 0 ? pad_w : -1;
  s.f32 = f32;
  s.Ho = (s.H + 2 * pad - KH) / stride + 1;
  s.Wo = (s.W + 2 * (pad_w >= 0 ? pad_w : pad) - KW) / (stride_w > 0 ? stride_w : stride) + 1;
  return s;
}
// implicit-GEMM rows and 64-deep k-steps of the forward, and of the data-grad (run as a forward
// convolution of dy), as the tuner's candidate lists need them
long conv_rows(const mipipe::ConvShape& s) { return (long)s.N * s.Ho * s.Wo; }
int conv_ksteps(const mipipe::ConvShape& s) { return (int)(((long)s.KH * s.KW * s.Ci + 63) / 64); }
long conv_dgrad_rows(const mipipe::ConvShape& s) { return (long)s.N * s.H * s.W; }
int conv_dgrad_ksteps(const mipipe::ConvShape& s) { return (int)(((long)s.KH * s.KW * s.Co + 63) / 64); }

mipipe::ConvShape conv_shape(const Tensor& x, const Tensor& w, int stride, int pad,
                             int stride_w = 0, int pad_w = -1) {
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "conv expects NHWC x and [Co,KH,KW,Ci] w");
  TORCH_CHECK(w.size(3) == x.size(3), "weight Ci ", w.size(3), " != input channels ", (int)x.size(3));
  TORCH_CHECK(stride >= 1 && pad >= 0, "bad stride/pad");
  const auto s = make_conv_shape(x.size(0), x.size(1), x.size(2), x.size(3), w.size(0),
                                 (int)w.size(1), (int)w.size(2), stride, pad, stride_w, pad_w,
                                 is_f32(x));
  TORCH_CHECK(s.Ho > 0 && s.Wo > 0, "empty conv output");
  TORCH_CHECK(s.Ci % 8 == 0, "conv kernels need Ci % 8 == 0 (pad channels), got ", s.Ci);
  TORCH_CHECK(x.numel() < (1ll << 31), "conv input too large for 32-bit gather offsets");
  TORCH_CHECK(s.Co % 8 == 0, "conv kernels need Co % 8 == 0, got ", s.Co);
  TORCH_CHECK((int64_t)s.N * s.H * s.W * s.Ci < (1ll << 31) &&
                  (int64_t)s.N * s.Ho * s.Wo * s.Co < (1ll << 31),
              "conv tensors beyond 2^31 elements are not supported");
  check_conv_buf_bytes(s, s.f32, "conv");
  return s;
}

// ------------------------------------------------------------------------------- tile tuning
// The cudnn.benchmark analogue (reference task.py:244 sets torch.backends.cudnn.benchmark):
// with benchmark mode on, the first call of a conv op on a new (op, shape, dtype) times every
// valid tile config on scratch outputs (hipEvents, eager stream only — never while a stream is
// being captured into a graph) and remembers the fastest; later calls reuse it.  The table can
// be exported / imported (mipipe.ops.tuning) so a job can ship a measured table.
namespace tune {
bool g_benchmark = false;
bool g_force_tune = false;  // time candidates even in deterministic mode (table generation)
bool g_verbose = false;
int g_reps = 3;
std::unordered_map<std::string, int> g_table;

std::string key(const char* op, const mipipe::ConvShape& s) {
  char buf[200];
  snprintf(buf, sizeof(buf), "%s|%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d|%s", op, s.N, s.H, s.W, s.Ci,
           s.Co, s.KH, s.KW, s.stride, s.pad, s.stride_w, s.pad_w, s.f32 ? "f32" : "bf16");
  return buf;
}

bool capturing() {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream(), &st) != hipSuccess) return true;
  return st != hipStreamCaptureStatusNone;
}

std::vector<int> candidates(bool f32, bool wgrad) {
  if (f32) return {0, 2, 8};
  // MIPIPE_CONV_TILES=n: tune over the first n tile configs only (A/B of added tiles)
  static const int ntiles = [] {
    const char* v = getenv("MIPIPE_CONV_TILES");
    const int n = v == nullptr ? mipipe::kConvTileConfigs : atoi(v);
    return n > 0 && n <= mipipe::kConvTileConfigs ? n : mipipe::kConvTileConfigs;
  }();
  std::vector<int> c;
  for (int i = 0; i < ntiles; ++i)
    if (!(wgrad && i == 6)) c.push_back(i);
  return c;
}

// cfg for this call: table hit, or (benchmark mode, not capturing) measure every candidate with
// `run(cfg)` (which must write only scratch outputs) and record the fastest; else -1 (heuristic).
template <class F>
int select_from(const std::string& k, const std::vector<int>& cands, F&& run) {
  auto it = g_table.find(k);
  if (it != g_table.end()) return it->second;
  if (!g_benchmark || capturing()) return -1;
  // Deterministic mode: the tile plan fixes the reduction partition (BatchNorm partial rows per
  // M tile, split-K slices), so a timing-based pick would make two runs sum in different
  // orders.  Only a loaded table (MIPIPE_TUNE_TABLE / the shipped one) or the heuristic decide,
  // unless tuning is forced (g_force_tune: building such a table).
  if (mipipe::g_deterministic && !g_force_tune) return -1;
  hipStream_t st = stream();
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  int best = -1;
  float best_ms = 1e30f;
  std::string log;
  // MIPIPE_TUNE_COLD=1: time every launch after a 512 MB sweep of the caches (operands as cold as
  // in a training step, where most were last touched a pass earlier) instead of back-to-back
  static const bool cold = env_flag("MIPIPE_TUNE_COLD", false);
  static void* sweep = nullptr;
  constexpr size_t kSweep = 512u << 20;
  if (cold && sweep == nullptr && hipMalloc(&sweep, kSweep) != hipSuccess) sweep = nullptr;
  for (int cfg : cands) {
    run(cfg);  // warm (first launch of a kernel object loads its code)
    float ms = 0.f;
    if (cold && sweep != nullptr) {
      for (int r = 0; r < g_reps; ++r) {
        hipMemsetAsync(sweep, r, kSweep, st);
        hipEventRecord(e0, st);
        run(cfg);
        hipEventRecord(e1, st);
        hipEventSynchronize(e1);
        float t = 0.f;
        hipEventElapsedTime(&t, e0, e1);
        ms += t;
      }
    } else {
      hipEventRecord(e0, st);
      for (int r = 0; r < g_reps; ++r) run(cfg);
      hipEventRecord(e1, st);
      hipEventSynchronize(e1);
      hipEventElapsedTime(&ms, e0, e1);
    }
    ms /= (float)g_reps;
    if (g_verbose) log += " " + std::to_string(cfg) + ":" + std::to_string(ms * 1e3f).substr(0, 7);
    if (ms < best_ms) {
      best_ms = ms;
      best = cfg;
    }
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  TORCH_CHECK(hipGetLastError() == hipSuccess, "tile tuning: a candidate failed to launch");
  if (g_verbose) fprintf(stderr, "[mipipe tune] %s -> %d  (us:%s)\n", k.c_str(), best, log.c_str());
  g_table[k] = best;
  return best;
}

template <class F>
int select(const std::string& k, bool f32, bool wgrad, F&& run) {
  return select_from(k, candidates(f32, wgrad), run);
}

// Conv forward / forward-style data-grad plans (plan.hpp decode_conv_plan): every tile, plus
// split-K plans of the tiles whose output tiles alone leave the chip under-filled (fewer than
// two blocks per CU; at least two k-steps per split).
std::vector<int> conv_plan_candidates(bool f32, long M, long N, int nk) {
  static const bool on = env_flag("MIPIPE_CONV_SPLIT", true);  // =0: no split-K plans (A/B)
  std::vector<int> c;
  for (int t : candidates(f32, false)) {
    c.push_back(t);
    if (!on) continue;
    int bm = 128, bn = 128;
    mipipe::conv_tile_dims(t, f32, &bm, &bn);
    if (bm == 256 && bn == 256 && t != 11) continue;  // the 4-wave 256x256 tile never splits
    const long tiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    if (tiles >= 512) continue;
    for (int sp : {2, 3, 4, 6, 8})
      if (nk >= 2 * sp && tiles * sp <= 4096) c.push_back(mipipe::encode_conv_plan(t, sp));
  }
  return c;
}

// GEMM plans (plan.hpp decode_gemm_plan): split counts for the accumulating GEMMs only
std::vector<int> gemm_candidates(bool f32, bool accumulate) {
  std::vector<int> c;
  for (int t : candidates(f32, accumulate)) {
    if (!accumulate) {
      c.push_back(t);
      continue;
    }
    for (int sp : {1, 2, 4}) c.push_back(mipipe::encode_gemm_plan(t, sp, false));
  }
  return c;
}
std::string gemm_key(int64_t M, int64_t N, int64_t K, bool akc, bool bkc, int mode, bool f32) {
  char buf[160];
  snprintf(buf, sizeof(buf), "gemm|%lld,%lld,%lld,%d,%d,%d|%s", (long long)M, (long long)N,
           (long long)K, (int)akc, (int)bkc, mode, f32 ? "f32" : "bf16");
  return buf;
}
}  // namespace tune

// ------------------------------------------------------------------------------- conv
std::tuple<Tensor, optional<Tensor>, optional<Tensor>> conv_fwd(Tensor x, Tensor w, int stride,
                                                                int pad, optional<Tensor> shift,
                                                                optional<Tensor> slab_sum,
                                                                optional<Tensor> slab_sq,
                                                                optional<Tensor> bias, bool relu,
                                                                int stride_w, int pad_w, int cfg,
                                                                optional<Tensor> wflip,
                                                                optional<Tensor> in_scale,
                                                                optional<Tensor> in_bias) {
  check_act(x, "x");
  check_same(w, x, "w");
  c10::DeviceGuard g(x.device());
  const auto s = conv_shape(x, w, stride, pad, stride_w, pad_w);
  // folded input BatchNorm: x holds y, the conv consumes relu(y*in_scale + in_bias)
  const float* isc = nullptr;
  const float* ibi = nullptr;
  if (in_scale.has_value()) {
    TORCH_CHECK(in_bias.has_value(), "in_scale needs in_bias");
    TORCH_CHECK(!s.f32 && mipipe::conv_is_dense(s) && s.Ci <= mipipe::kConvBnInMaxK && !wflip.has_value(),
                "folded input BN: bf16 dense 1x1 stride-1 convs with Ci <= ", mipipe::kConvBnInMaxK);
    check_vec(*in_scale, s.Ci, "in_scale");
    check_vec(*in_bias, s.Ci, "in_bias");
    isc = in_scale->data_ptr<float>();
    ibi = in_bias->data_ptr<float>();
  }
  // wflip: the launch also writes the tap-flipped weight of this conv's stride-1 data-grad
  void* wfp = nullptr;
  if (wflip.has_value() && mipipe::dgrad_preflip_ok(s)) {
    check_same(*wflip, w, "wflip");
    TORCH_CHECK(wflip->numel() == w.numel() && wflip->is_contiguous(), "wflip must match w's size");
    wfp = wflip->data_ptr();
  }
  if (bias.has_value()) check_vec(*bias, s.Co, "bias");
  TORCH_CHECK(!(shift.has_value() && (bias.has_value() || relu)),
              "BN-statistics epilogue and bias/ReLU epilogue are exclusive");
  auto y = torch::empty({s.N, s.Ho, s.Wo, s.Co}, x.options());
  optional<Tensor> ps, pss;
  float *psp = nullptr, *pssp = nullptr;
  const float* sh = nullptr;
  if (shift.has_value()) {
    check_vec(*shift, s.Co, "stats_shift");
    int P = mipipe::conv_fwd_stat_rows(s);
    if (slab_sum.has_value()) {  // persistent zeroed replica slabs (re-zeroed by bn_finalize)
      check_f32(*slab_sum, "slab_sum");
      check_f32(*slab_sq, "slab_sq");
      TORCH_CHECK(slab_sum->numel() == (int64_t)P * s.Co && slab_sq->numel() == (int64_t)P * s.Co,
                  "stat slabs must be [", P, ", Co]");
      ps = *slab_sum;
      pss = *slab_sq;
    } else {
      ps = torch::zeros({P, s.Co}, x.options().dtype(at::kFloat));
      pss = torch::zeros({P, s.Co}, x.options().dtype(at::kFloat));
    }
    psp = ps->data_ptr<float>();
    pssp = pss->data_ptr<float>();
    sh = shift->data_ptr<float>();
  }
  const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  if (cfg < 0) {
    std::vector<int> cands = tune::conv_plan_candidates(s.f32, conv_rows(s), s.Co, conv_ksteps(s));
    if (isc != nullptr) {  // folded-BN variant: 4-wave tiles, no split
      cands.clear();
      for (int t : tune::candidates(false, false))
        if (t < 11) cands.push_back(t);
    }
    cfg = tune::select_from(tune::key(isc != nullptr ? "fwdbn" : "fwd", s), cands, [&](int c) {
      auto ys = torch::empty_like(y);
      optional<Tensor> a, b;
      if (psp != nullptr) {
        a = torch::zeros_like(*ps);
        b = torch::zeros_like(*pss);
      }
      Tensor ws = split_ws(mipipe::conv_fwd_split_ws_elems(s, c), x);
      mipipe::conv_fwd(x.data_ptr(), w.data_ptr(), ys.data_ptr(),
                       a.has_value() ? a->data_ptr<float>() : nullptr,
                       b.has_value() ? b->data_ptr<float>() : nullptr, sh, s, stream(), bp, relu, c,
                       0, nullptr, wsp(ws), isc, ibi);
    });
  }
  if (isc != nullptr && mipipe::decode_conv_plan(cfg).tile >= 11) cfg = -1;  // (a table from elsewhere)
  Tensor ws = split_ws(mipipe::conv_fwd_split_ws_elems(s, cfg), x);
  if (mipipe::g_deterministic && psp != nullptr) {
    // per-M-tile partial rows (no atomics), then a fixed-order sum into slab row 0; the other
    // replica rows of the slabs stay zero
    const int P = mipipe::conv_fwd_tiles_m(s, cfg);
    auto part = torch::empty({2, P, s.Co}, x.options().dtype(at::kFloat));
    float* p0 = part.data_ptr<float>();
    mipipe::conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), p0, p0 + (long)P * s.Co, sh, s,
                     stream(), bp, relu, cfg, P, wfp, wsp(ws), isc, ibi);
    // the partial rows themselves go to bn_finalize, which sums them in det_sum_rows' fixed
    // order (chunk sums first for long columns) — no separate summing launch into the slab
    (void)psp;
    return {y, part[0], part[1]};
  }
  mipipe::conv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), psp, pssp, sh, s, stream(), bp, relu,
                   cfg, 0, wfp, wsp(ws), isc, ibi);
  return {y, ps, pss};
}

// Inference forward: y = act(conv(x, w) * scale + shift + residual) in the conv's epilogue
// (conv_infer.hip) — an eval-mode BatchNorm folded to (scale, shift) by bn_fold_affine, the
// block's residual and its ReLU.  Plans are tuned under their own keys: the candidates are the
// plain forward's, the epilogue (and so the best tile) is not.
Tensor conv_fwd_infer(Tensor x, Tensor w, int stride, int pad, optional<Tensor> scale,
                      optional<Tensor> shift, optional<Tensor> residual, bool relu, int stride_w,
                      int pad_w, int cfg) {
  check_act(x, "x");
  check_same(w, x, "w");
  c10::DeviceGuard g(x.device());
  const auto s = conv_shape(x, w, stride, pad, stride_w, pad_w);
  auto vec = [&](const optional<Tensor>& t, const char* name) -> const float* {
    if (!t.has_value()) return nullptr;
    check_vec(*t, s.Co, name);
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
    return t->data_ptr<float>();
  };
  const float* scp = vec(scale, "scale");
  const float* shp = vec(shift, "shift");
  auto y = torch::empty({s.N, s.Ho, s.Wo, s.Co}, x.options());
  const void* rp = nullptr;
  if (residual.has_value()) {
    check_same(*residual, x, "residual");
    TORCH_CHECK(residual->sizes() == y.sizes(), "residual must have the output's shape ", y.sizes(),
                ", got ", residual->sizes());
    rp = residual->data_ptr();
  }
  if (cfg < 0) {
    cfg = tune::select_from(tune::key(rp != nullptr ? "fwdinfr" : "fwdinf", s),
                            tune::conv_plan_candidates(s.f32, conv_rows(s), s.Co, conv_ksteps(s)),
                            [&](int c) {
      auto ys = torch::empty_like(y);
      Tensor ws = split_ws(mipipe::conv_fwd_split_ws_elems(s, c), x);
      mipipe::conv_fwd_infer(x.data_ptr(), w.data_ptr(), ys.data_ptr(), s, stream(), scp, shp, rp,
                             relu, c, wsp(ws));
    });
  }
  Tensor ws = split_ws(mipipe::conv_fwd_split_ws_elems(s, cfg), x);
  mipipe::conv_fwd_infer(x.data_ptr(), w.data_ptr(), y.data_ptr(), s, stream(), scp, shp, rp, relu,
                         cfg, wsp(ws));
  return y;
}

Tensor conv_dgrad(Tensor dy, Tensor w, std::vector<int64_t> x_shape, int stride, int pad,
                  optional<Tensor> addend, optional<Tensor> bn_y, optional<Tensor> bn_mean,
                  optional<Tensor> bn_invstd, optional<Tensor> bn_scale, optional<Tensor> bn_bias,
                  optional<Tensor> bn_rep, optional<Tensor> bn_z, int pad_w, int cfg,
                  optional<Tensor> bn_mask, optional<Tensor> bn_y2, optional<Tensor> bn_mean2,
                  optional<Tensor> bn_invstd2, optional<Tensor> wflip_pre) {
  check_act(dy, "dy");
  check_same(w, dy, "w");
  c10::DeviceGuard g(dy.device());
  TORCH_CHECK(x_shape.size() == 4, "x_shape must be [N,H,W,Ci]");
  // (the data-grad has no horizontal stride of its own: stride_w stays 0)
  const auto s = make_conv_shape(x_shape[0], x_shape[1], x_shape[2], x_shape[3], w.size(0),
                                 (int)w.size(1), (int)w.size(2), stride, pad, 0, pad_w, is_f32(dy));
  TORCH_CHECK(w.size(3) == s.Ci, "weight/input channel mismatch");
  const int pw = pad_w >= 0 ? pad_w : pad;
  TORCH_CHECK(dy.size(0) == s.N && dy.size(1) == s.Ho && dy.size(2) == s.Wo && dy.size(3) == s.Co,
              "dy shape does not match the convolution");
  TORCH_CHECK(s.Ci % 8 == 0 && s.Co % 8 == 0, "conv dgrad needs Ci, Co % 8 == 0");
  TORCH_CHECK(dy.numel() < (1ll << 31), "conv dgrad dy too large for 32-bit gather offsets");
  check_conv_buf_bytes(s, s.f32, "conv dgrad");
  TORCH_CHECK(s.pad < s.KH && pw < s.KW, "conv dgrad expects padding < kernel size");
  auto dx = torch::empty({s.N, s.H, s.W, s.Ci}, dy.options());
  // data-grads run as forward convolutions over tap-flipped (sub-)kernels, per stride-parity
  // class; MIPIPE_DGRAD_FWD=0: the data-grad gather kernels everywhere, =2: also 1x1 stride-1
  const int fwd_style_mode = mipipe::dgrad_fwd_style_mode();
  Tensor wflip;
  void* wfp = nullptr;
  bool preflipped = false;
  if (fwd_style_mode > 0 && mipipe::conv_dgrad_fwd_style(s, fwd_style_mode >= 2) &&
      !bn_y2.has_value()) {
    if (wflip_pre.has_value() && mipipe::dgrad_preflip_ok(s)) {
      // written by this conv's forward launch (conv_fwd's wflip): no flip kernel here
      check_same(*wflip_pre, w, "wflip_pre");
      TORCH_CHECK(wflip_pre->numel() == w.numel() && wflip_pre->is_contiguous(),
                  "wflip_pre must match w's size");
      wfp = wflip_pre->data_ptr();
      preflipped = true;
    } else {
      wflip = torch::empty({(int64_t)s.Ci * s.KH * s.KW * s.Co}, w.options());  // w: [Co,KH,KW,Ci]
      wfp = wflip.data_ptr();
    }
  }
  mipipe::DgradFusion fz;
  bool any = false;
  if (addend.has_value()) {
    check_same(*addend, dy, "addend");
    TORCH_CHECK(addend->sizes() == dx.sizes(), "addend must match dx");
    fz.addend = addend->data_ptr();
    any = true;
  }
  if (bn_rep.has_value()) {
    TORCH_CHECK(bn_y.has_value() && bn_mean.has_value() && bn_invstd.has_value() &&
                bn_scale.has_value() && bn_bias.has_value(), "BN fusion needs y/mean/invstd/scale/bias");
    check_same(*bn_y, dy, "bn_y");
    TORCH_CHECK(bn_y->sizes() == dx.sizes(), "bn_y must match dx");
    check_vec(*bn_mean, s.Ci, "bn_mean");
    check_vec(*bn_invstd, s.Ci, "bn_invstd");
    check_vec(*bn_scale, s.Ci, "bn_scale");
    check_vec(*bn_bias, s.Ci, "bn_bias");
    check_f32(*bn_rep, "bn_rep");
    TORCH_CHECK(bn_rep->numel() == 3ll * mipipe::kStatReplicas * s.Ci, "bn_rep must be [3,R,Ci]");
    for (const Tensor* t : {&*bn_mean, &*bn_invstd, &*bn_scale, &*bn_bias})
      TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                  "BN fusion vectors must be 16-byte aligned (the epilogue reads them as float4)");
    fz.bn_y = bn_y->data_ptr();
    fz.bn_mean = bn_mean->data_ptr<float>(); fz.bn_invstd = bn_invstd->data_ptr<float>();
    fz.bn_scale = bn_scale->data_ptr<float>(); fz.bn_bias = bn_bias->data_ptr<float>();
    fz.bn_rep = bn_rep->data_ptr<float>();
    if (bn_mask.has_value()) {  // the ReLU mask as bits, written by bn_act_fwd
      check_cuda(*bn_mask, "bn_mask");
      TORCH_CHECK(bn_mask->scalar_type() == at::kByte && bn_mask->is_contiguous() &&
                      bn_mask->numel() * 8 == dx.numel(), "bn_mask must be uint8 [rows, Ci/8]");
      fz.bn_mask = bn_mask->data_ptr<uint8_t>();
    }
    if (bn_z.has_value()) {
      check_same(*bn_z, dy, "bn_z");
      TORCH_CHECK(bn_z->sizes() == dx.sizes(), "bn_z must match dx");
      fz.bn_z = bn_z->data_ptr();
    }
    if (bn_y2.has_value()) {  // two-branch block output: relu(bn(y) + bn2(y2))
      TORCH_CHECK(bn_mean2.has_value() && bn_invstd2.has_value(), "bn_y2 needs mean2/invstd2");
      TORCH_CHECK(!s.f32 && s.KH == 1 && s.KW == 1 && stride == 1 && pad == 0 && pw == 0,
                  "two-branch BN fusion: bf16 1x1 stride-1 data-grads only");
      check_same(*bn_y2, dy, "bn_y2");
      TORCH_CHECK(bn_y2->sizes() == dx.sizes(), "bn_y2 must match dx");
      check_vec(*bn_mean2, s.Ci, "bn_mean2");
      check_vec(*bn_invstd2, s.Ci, "bn_invstd2");
      for (const Tensor* t : {&*bn_mean2, &*bn_invstd2})
        TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                    "BN fusion vectors must be 16-byte aligned");
      fz.bn_y2 = bn_y2->data_ptr();
      fz.bn_mean2 = bn_mean2->data_ptr<float>();
      fz.bn_invstd2 = bn_invstd2->data_ptr<float>();
    }
    any = true;
  }
  // split-K plans apply to the forward-style classes only (they need the flipped weight)
  auto dgrad_ws = [&](int plan) {
    return split_ws(wfp != nullptr ? mipipe::conv_dgrad_split_ws_elems(s, plan) : 0, dy);
  };
  if (cfg < 0) {
    std::vector<int> cands = tune::candidates(s.f32, false);
    if (wfp != nullptr && s.stride == 1)
      cands = tune::conv_plan_candidates(s.f32, conv_dgrad_rows(s), s.Ci, conv_dgrad_ksteps(s));
    cfg = tune::select_from(tune::key("dgrad", s), cands, [&](int c) {
      auto dxs = torch::empty_like(dx);
      mipipe::DgradFusion f2 = fz;
      Tensor reps;
      if (fz.bn_rep != nullptr) {
        reps = torch::zeros_like(*bn_rep);
        f2.bn_rep = reps.data_ptr<float>();
      }
      Tensor ws = dgrad_ws(c);
      mipipe::conv_dgrad(dy.data_ptr(), w.data_ptr(), dxs.data_ptr(), s, stream(),
                         any ? &f2 : nullptr, c, wfp, preflipped, wsp(ws));
    });
  }
  Tensor ws = dgrad_ws(cfg);
  if (mipipe::g_deterministic && fz.bn_rep != nullptr) {
    const int P = mipipe::conv_dgrad_tiles_m(s, cfg);
    const bool two = fz.bn_y2 != nullptr;
    auto part = torch::empty({two ? 3 : 2, P, s.Ci}, dy.options().dtype(at::kFloat));
    float* rep = fz.bn_rep;
    fz.bn_rep = part.data_ptr<float>();
    fz.det_rows = P;
    mipipe::conv_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), s, stream(), &fz, cfg, wfp,
                       preflipped, wsp(ws));
    const long rs = (long)mipipe::kStatReplicas * s.Ci, ps = (long)P * s.Ci;
    mipipe::det_sum_rows(fz.bn_rep, fz.bn_rep + ps, P, s.Ci, rep, rep + rs, false, stream());
    if (two)
      mipipe::det_sum_rows(fz.bn_rep + 2 * ps, nullptr, P, s.Ci, rep + 2 * rs, nullptr, false,
                           stream());
    return dx;
  }
  mipipe::conv_dgrad(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), s, stream(), any ? &fz : nullptr,
                     cfg, wfp, preflipped, wsp(ws));
  return dx;
}

std::tuple<Tensor, Tensor> bn_bwd_collect(Tensor rep, int64_t C, optional<Tensor> dgamma,
                                          optional<Tensor> dbeta) {
  check_f32(rep, "rep");
  c10::DeviceGuard g(rep.device());
  TORCH_CHECK(rep.numel() == 3ll * mipipe::kStatReplicas * C, "rep must be [3,R,C]");
  TORCH_CHECK(dgamma.has_value() == dbeta.has_value(), "pass both accumulators or none");
  auto o = rep.options();
  auto sg = torch::empty({C}, o), sgx = torch::empty({C}, o);
  mipipe::bn_bwd_collect(rep.data_ptr<float>(), (int)C, sg.data_ptr<float>(), sgx.data_ptr<float>(),
                         fptr(dgamma, C), fptr(dbeta, C), stream());
  return {sg, sgx};
}

Tensor conv_wgrad(Tensor dy, Tensor x, int kh, int kw, int stride, int pad, optional<Tensor> out,
                  int stride_w, int pad_w, int cfg, optional<Tensor> col_rep,
                  optional<Tensor> col_out, optional<Tensor> col_dgamma,
                  optional<Tensor> col_dbeta, bool col_two, optional<Tensor> col_dgamma2,
                  optional<Tensor> col_dbeta2, optional<Tensor> in_scale,
                  optional<Tensor> in_bias) {
  check_act(dy, "dy");
  check_same(x, dy, "x");
  c10::DeviceGuard g(dy.device());
  const auto s = make_conv_shape(x.size(0), x.size(1), x.size(2), x.size(3), dy.size(3), kh, kw,
                                 stride, pad, stride_w, pad_w, is_f32(dy));
  TORCH_CHECK(x.numel() < (1ll << 31), "conv wgrad input too large for 32-bit gather offsets");
  TORCH_CHECK(dy.size(0) == s.N && dy.size(1) == s.Ho && dy.size(2) == s.Wo, "dy/x mismatch");
  TORCH_CHECK(s.Ci % 8 == 0 && s.Co % 8 == 0, "conv wgrad needs Ci, Co % 8 == 0");
  check_conv_buf_bytes(s, s.f32, "conv wgrad");
  const float* isc = nullptr;  // folded input BN (see conv_fwd)
  const float* ibi = nullptr;
  if (in_scale.has_value()) {
    TORCH_CHECK(in_bias.has_value(), "in_scale needs in_bias");
    TORCH_CHECK(!s.f32 && mipipe::conv_is_dense(s), "folded input BN: bf16 dense 1x1 stride-1 convs");
    check_vec(*in_scale, s.Ci, "in_scale");
    check_vec(*in_bias, s.Ci, "in_bias");
    isc = in_scale->data_ptr<float>();
    ibi = in_bias->data_ptr<float>();
  }
  Tensor dw;
  if (out.has_value()) {  // accumulate straight into an existing gradient (flat DDP bucket view)
    check_f32(*out, "out");
    TORCH_CHECK(out->dim() == 4 && out->size(0) == s.Co && out->size(1) == kh && out->size(2) == kw &&
                    out->size(3) == s.Ci, "wgrad out must be [Co,KH,KW,Ci]");
    dw = *out;
  } else {
    dw = torch::zeros({s.Co, kh, kw, s.Ci}, x.options().dtype(at::kFloat));
  }
  // optional BN-backward collect riding in the launch (bn_bwd_collect's work, BnCollect)
  mipipe::BnCollect col;
  const mipipe::BnCollect* colp = nullptr;
  if (col_rep.has_value()) {
    check_f32(*col_rep, "col_rep");
    const int64_t C = col_rep->numel() / (3ll * mipipe::kStatReplicas);
    TORCH_CHECK(col_rep->numel() == 3ll * mipipe::kStatReplicas * C, "col_rep must be [3,R,C]");
    TORCH_CHECK(col_out.has_value(), "col_out needed");
    check_f32(*col_out, "col_out");
    TORCH_CHECK(col_out->numel() == (col_two ? 3 : 2) * C && col_out->is_contiguous(),
                "col_out must be [2,C] ([3,C] with col_two)");
    TORCH_CHECK(col_dgamma.has_value() == col_dbeta.has_value(), "pass both accumulators or none");
    TORCH_CHECK(col_dgamma2.has_value() == col_dbeta2.has_value(), "pass both accumulators or none");
    col.rep = col_rep->data_ptr<float>();
    col.C = (int)C;
    col.out = col_out->data_ptr<float>();
    col.dgamma = fptr(col_dgamma, C);
    col.dbeta = fptr(col_dbeta, C);
    col.two = col_two;
    col.dgamma2 = fptr(col_dgamma2, C);
    col.dbeta2 = fptr(col_dbeta2, C);
    colp = &col;
  }
  // 3x3 / stride-1 convolutions: the patch-resident kernel (input patch in LDS shared by the
  // 9 taps, partial tiles summed in a fixed order: deterministic in both modes)
  if (cfg < 0 && isc == nullptr && mipipe::g_wgrad3x3 && mipipe::conv_wgrad3x3_supported(s)) {
    const int S = mipipe::conv_wgrad3x3_splits(s);
    auto ws = torch::empty({S, (int64_t)s.Co * 9 * s.Ci}, dy.options().dtype(at::kFloat));
    mipipe::conv_wgrad3x3(dy.data_ptr(), x.data_ptr(), dw.data_ptr<float>(), s, stream(),
                          ws.data_ptr<float>(), S, colp);
    return dw;
  }
  // a gemm plan (plan.hpp).  Plan::ws, and every split in deterministic mode: the split partial
  // tiles go to workspace slices summed in order instead of fp32 atomics — cheaper where
  // splits x Co x K x 4 B of atomics would run at ~1.3 TB/s
  auto launch = [&](float* out, const mipipe::Plan& p, const mipipe::BnCollect* c) {
    const int splits = mipipe::conv_wgrad_splits(s, p.tile, p.splits);
    if (splits == 1) {  // one writer per element: the plain read-modify-write is deterministic
      mipipe::conv_wgrad(dy.data_ptr(), x.data_ptr(), out, s, stream(), p.tile, nullptr, 1, c, isc,
                         ibi);
      return;
    }
    auto ws = torch::empty({splits, (int64_t)s.Co * kh * kw * s.Ci}, dy.options().dtype(at::kFloat));
    mipipe::conv_wgrad(dy.data_ptr(), x.data_ptr(), out, s, stream(), p.tile, ws.data_ptr<float>(),
                       p.splits, c, isc, ibi);
  };
  auto launch_atomic = [&](float* out, const mipipe::Plan& p, const mipipe::BnCollect* c) {
    mipipe::conv_wgrad(dy.data_ptr(), x.data_ptr(), out, s, stream(), p.tile, nullptr, p.splits, c,
                       isc, ibi);
  };
  if (cfg < 0) {
    // 3 / 6 / 12 / 24 splits as well: tiles x splits lands nearer a whole number of waves
    // (MIPIPE_WGRAD_WIDE_SPLITS=0: powers of two only, A/B)
    static const bool wide = env_flag("MIPIPE_WGRAD_WIDE_SPLITS", true);
    static const bool ws_cands = env_flag("MIPIPE_WGRAD_WS", true);  // =0: atomic split-K only (A/B)
    std::vector<int> cands;
    for (int t : tune::candidates(s.f32, true)) {
      if (isc != nullptr && t >= 11) continue;  // folded-BN variant: 4-wave tiles
      for (int sp : {0, 1, 2, 3, 4, 6, 8, 12, 16})
        if (wide || (sp & (sp - 1)) == 0) cands.push_back(mipipe::encode_gemm_plan(t, sp, false));
      if (!mipipe::g_deterministic && ws_cands)
        for (int sp : {4, 6, 8, 12, 16, 24, 32})
          if (wide || (sp & (sp - 1)) == 0) cands.push_back(mipipe::encode_gemm_plan(t, sp, true));
    }
    cfg = tune::select_from(tune::key(isc != nullptr ? "wgradbn" : "wgrad", s), cands, [&](int c) {
      auto dws = torch::zeros_like(dw);
      const mipipe::Plan p = mipipe::decode_gemm_plan(c, false);
      // collect off while timing (col rides in the real launch only)
      if (p.ws) launch(dws.data_ptr<float>(), p, nullptr);
      else launch_atomic(dws.data_ptr<float>(), p, nullptr);
    });
  }
  const mipipe::Plan plan = mipipe::decode_gemm_plan(cfg, false);
  if (plan.ws || mipipe::g_deterministic) launch(dw.data_ptr<float>(), plan, colp);
  else launch_atomic(dw.data_ptr<float>(), plan, colp);
  return dw;
}

// ------------------------------------------------------------------------------- batchnorm
std::tuple<Tensor, Tensor, Tensor, Tensor> bn_finalize(Tensor psum, Tensor psq, int64_t count,
                                                       Tensor shift, Tensor gamma, Tensor beta,
                                                       optional<Tensor> rm, optional<Tensor> rv,
                                                       double momentum, double eps,
                                                       bool zero_after, optional<Tensor> nbt) {
  check_f32(psum, "psum");
  check_f32(psq, "psumsq");
  c10::DeviceGuard g(psum.device());
  int64_t C = psum.size(-1);
  int64_t P = psum.numel() / C;
  check_vec(shift, C, "shift");
  check_vec(gamma, C, "gamma");
  check_vec(beta, C, "beta");
  if (rm.has_value()) {
    check_vec(*rm, C, "running_mean");
    check_vec(*rv, C, "running_var");
  }
  long long* nbt_p = nullptr;
  if (nbt.has_value()) {
    TORCH_CHECK(nbt->scalar_type() == at::kLong && nbt->numel() == 1 && nbt->is_cuda(),
                "num_batches_tracked: int64 scalar on the GPU");
    nbt_p = reinterpret_cast<long long*>(nbt->data_ptr<int64_t>());
  }
  auto st4 = torch::empty({4, C}, psum.options());  // one allocation: mean/invstd/scale/bias
  auto mean = st4[0], invstd = st4[1], scale = st4[2], bias = st4[3];
  mipipe::bn_finalize(psum.data_ptr<float>(), psq.data_ptr<float>(), (int)P, (int)C, count,
                      shift.data_ptr<float>(), gamma.data_ptr<float>(), beta.data_ptr<float>(),
                      rm.has_value() ? rm->data_ptr<float>() : nullptr,
                      rv.has_value() ? rv->data_ptr<float>() : nullptr, (float)momentum,
                      (float)eps, mean.data_ptr<float>(), invstd.data_ptr<float>(),
                      scale.data_ptr<float>(), bias.data_ptr<float>(), zero_after, nbt_p,
                      stream());
  return {mean, invstd, scale, bias};
}

// Eval-mode BatchNorm (+ the producing conv's bias) as (scale, shift), one launch
std::tuple<Tensor, Tensor> bn_fold_affine(Tensor gamma, Tensor beta, Tensor rm, Tensor rv,
                                          double eps, optional<Tensor> conv_bias) {
  check_f32(gamma, "weight");
  c10::DeviceGuard g(gamma.device());
  const int64_t C = gamma.numel();
  check_vec(beta, C, "bias");
  check_vec(rm, C, "running_mean");
  check_vec(rv, C, "running_var");
  if (conv_bias.has_value()) check_vec(*conv_bias, C, "conv_bias");
  // one allocation, rows 16-B aligned for the conv epilogue's vector loads
  const int64_t Cp = (C + 3) / 4 * 4;
  auto st2 = torch::empty({2, Cp}, gamma.options());
  auto scale = st2[0].narrow(0, 0, C), shift = st2[1].narrow(0, 0, C);
  mipipe::bn_fold_affine(gamma.data_ptr<float>(), beta.data_ptr<float>(), rm.data_ptr<float>(),
                         rv.data_ptr<float>(),
                         conv_bias.has_value() ? conv_bias->data_ptr<float>() : nullptr, (float)eps,
                         (int)C, scale.data_ptr<float>(), shift.data_ptr<float>(), stream());
  return {scale, shift};
}

Tensor bn_act_fwd(Tensor y, Tensor scale, Tensor bias, bool relu, optional<Tensor> r,
                  optional<Tensor> rscale, optional<Tensor> rbias, optional<Tensor> mask) {
  check_act(y, "y");
  c10::DeviceGuard g(y.device());
  TORCH_CHECK(y.numel() > 0, "bn_act_fwd: empty input");
  int64_t C = y.size(-1), M = y.numel() / C;
  TORCH_CHECK(C % 8 == 0, "bn_act_fwd needs C % 8 == 0");
  check_vec(scale, C, "scale");
  check_vec(bias, C, "bias");
  if (r.has_value()) {
    check_same(*r, y, "residual");
    TORCH_CHECK(r->sizes() == y.sizes(), "residual shape mismatch");
  }
  if (rscale.has_value()) {
    check_vec(*rscale, C, "res_scale");
    check_vec(*rbias, C, "res_bias");
  }
  uint8_t* mp = nullptr;
  if (mask.has_value()) {  // also write the ReLU mask of z as bits
    check_cuda(*mask, "mask");
    TORCH_CHECK(mask->scalar_type() == at::kByte && mask->is_contiguous() &&
                    mask->numel() * 8 == y.numel(), "mask must be uint8 [rows, C/8]");
    mp = mask->data_ptr<uint8_t>();
  }
  auto z = torch::empty_like(y);
  mipipe::bn_act_fwd(y.data_ptr(), scale.data_ptr<float>(), bias.data_ptr<float>(), ptr_or_null(r),
                     rscale.has_value() ? rscale->data_ptr<float>() : nullptr,
                     rbias.has_value() ? rbias->data_ptr<float>() : nullptr, z.data_ptr(), M,
                     (int)C, relu, stream(), is_f32(y), mp);
  return z;
}

std::tuple<Tensor, Tensor, optional<Tensor>> bn_act_bwd_reduce(
    Tensor dz, Tensor z, Tensor y, Tensor mean, Tensor invstd, bool relu, optional<Tensor> y2,
    optional<Tensor> mean2, optional<Tensor> invstd2, optional<Tensor> rep,
    optional<Tensor> dgamma, optional<Tensor> dbeta, optional<Tensor> dgamma2,
    optional<Tensor> dbeta2) {
  check_act(y, "y");
  check_same(dz, y, "dz");
  check_same(z, y, "z");
  c10::DeviceGuard g(dz.device());
  TORCH_CHECK(y.numel() > 0, "bn_act_bwd_reduce: empty input");
  int64_t C = y.size(-1), M = y.numel() / C;
  TORCH_CHECK(C % 8 == 0 && dz.sizes() == y.sizes() && z.sizes() == y.sizes(), "shape mismatch");
  check_vec(mean, C, "mean");
  check_vec(invstd, C, "invstd");
  if (y2.has_value()) {
    check_same(*y2, y, "y2");
    TORCH_CHECK(y2->sizes() == y.sizes(), "y2 shape mismatch");
    check_vec(*mean2, C, "mean2");
    check_vec(*invstd2, C, "invstd2");
  }
  auto o = y.options().dtype(at::kFloat);
  auto sg = torch::empty({C}, o), sgx = torch::empty({C}, o);
  optional<Tensor> sgx2;
  if (y2.has_value()) sgx2 = torch::empty({C}, o);
  Tensor work;
  if (rep.has_value()) {  // persistent zeroed [3][R][C] replica slab, left zeroed
    check_f32(*rep, "rep");
    TORCH_CHECK(rep->numel() == 3L * mipipe::kStatReplicas * C, "rep must be [3, R, C]");
    work = *rep;
  } else {
    work = torch::zeros({3L * mipipe::kStatReplicas * C}, o);
  }
  optional<Tensor> det_ws;
  if (mipipe::g_deterministic)
    det_ws = torch::empty({3, (int64_t)mipipe::bn_bwd_reduce_blocks(M, (int)C), C}, o);
  mipipe::bn_act_bwd_reduce(dz.data_ptr(), z.data_ptr(), y.data_ptr(), mean.data_ptr<float>(),
                            invstd.data_ptr<float>(), ptr_or_null(y2),
                            mean2.has_value() ? mean2->data_ptr<float>() : nullptr,
                            invstd2.has_value() ? invstd2->data_ptr<float>() : nullptr, relu, M,
                            (int)C, sg.data_ptr<float>(), sgx.data_ptr<float>(),
                            sgx2.has_value() ? sgx2->data_ptr<float>() : nullptr,
                            work.data_ptr<float>(), fptr(dgamma, C), fptr(dbeta, C),
                            fptr(dgamma2, C), fptr(dbeta2, C), stream(), is_f32(y),
                            det_ws.has_value() ? det_ws->data_ptr<float>() : nullptr);
  return {sg, sgx, sgx2};
}

std::tuple<Tensor, optional<Tensor>> bn_act_bwd_apply(
    Tensor dz, Tensor z, Tensor y, Tensor mean, Tensor invstd, Tensor gamma, Tensor sum_g,
    Tensor sum_gx, int64_t count, bool relu, bool want_dres, optional<Tensor> y2,
    optional<Tensor> mean2, optional<Tensor> invstd2, optional<Tensor> gamma2,
    optional<Tensor> sum_gx2) {
  check_act(y, "y");
  check_same(dz, y, "dz");
  check_same(z, y, "z");
  c10::DeviceGuard g(dz.device());
  TORCH_CHECK(y.numel() > 0, "bn_act_bwd_apply: empty input");
  int64_t C = y.size(-1), M = y.numel() / C;
  TORCH_CHECK(C % 8 == 0 && dz.sizes() == y.sizes() && z.sizes() == y.sizes(), "shape mismatch");
  for (auto* t : {&mean, &invstd, &gamma, &sum_g, &sum_gx}) check_vec(*t, C, "bn vector");
  if (y2.has_value()) {
    check_same(*y2, y, "y2");
    TORCH_CHECK(y2->sizes() == y.sizes(), "y2 shape mismatch");
    check_vec(*mean2, C, "mean2");
    check_vec(*invstd2, C, "invstd2");
    check_vec(*gamma2, C, "gamma2");
    check_vec(*sum_gx2, C, "sum_gx2");
  }
  auto dy = torch::empty_like(y);
  optional<Tensor> other;
  if (y2.has_value() || want_dres) other = torch::empty_like(y);
  mipipe::bn_act_bwd_apply(
      dz.data_ptr(), z.data_ptr(), y.data_ptr(), mean.data_ptr<float>(), invstd.data_ptr<float>(),
      gamma.data_ptr<float>(), sum_g.data_ptr<float>(), sum_gx.data_ptr<float>(), ptr_or_null(y2),
      mean2.has_value() ? mean2->data_ptr<float>() : nullptr,
      invstd2.has_value() ? invstd2->data_ptr<float>() : nullptr,
      gamma2.has_value() ? gamma2->data_ptr<float>() : nullptr,
      sum_gx2.has_value() ? sum_gx2->data_ptr<float>() : nullptr, count, relu, want_dres,
      dy.data_ptr(), other.has_value() ? other->data_ptr() : nullptr, M, (int)C, stream(),
      is_f32(y));
  return {dy, other};
}

// ------------------------------------------------------------------------------- pooling
std::tuple<Tensor, Tensor> maxpool_fwd(Tensor x, int k, int s, int p, bool ceil_mode) {
  check_act(x, "x");
  c10::DeviceGuard g(x.device());
  int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  TORCH_CHECK(C % 8 == 0 && k <= 15, "maxpool needs C % 8 == 0 and k <= 15");
  TORCH_CHECK(k >= 1 && s >= 1 && p >= 0 && 2 * p <= k, "bad maxpool geometry");
  int Ho = pool_out(H, k, s, p, ceil_mode), Wo = pool_out(W, k, s, p, ceil_mode);
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty maxpool output");
  auto y = torch::empty({N, Ho, Wo, C}, x.options());
  auto idx = torch::empty({N, Ho, Wo, C}, x.options().dtype(at::kByte));
  mipipe::maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr<uint8_t>(), N, H, W, C, Ho, Wo, k, s,
                      p, stream(), is_f32(x));
  return {y, idx};
}

// Stem fusion: max-pool of relu(y*scale + bias) without storing the normalised activation.
std::tuple<Tensor, Tensor> pool_bn_fwd(Tensor y, Tensor scale, Tensor bias, int k, int s, int p) {
  check_act(y, "y");
  c10::DeviceGuard g(y.device());
  int N = y.size(0), H = y.size(1), W = y.size(2), C = y.size(3);
  TORCH_CHECK(C % 8 == 0 && 256 % (C / 8) == 0 && k <= 15, "pool_bn: C % 8 == 0, 256 % (C/8) == 0");
  TORCH_CHECK(k >= 1 && s >= 1 && p >= 0 && 2 * p <= k, "bad maxpool geometry");
  check_vec(scale, C, "scale");
  check_vec(bias, C, "bias");
  for (const Tensor* t : {&scale, &bias})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "pool_bn vectors: 16-B aligned");
  int Ho = pool_out(H, k, s, p, false), Wo = pool_out(W, k, s, p, false);
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty maxpool output");
  auto out = torch::empty({N, Ho, Wo, C}, y.options());
  auto idx = torch::empty({N, Ho, Wo, C}, y.options().dtype(at::kByte));
  mipipe::pool_bn_fwd(y.data_ptr(), scale.data_ptr<float>(), bias.data_ptr<float>(), out.data_ptr(),
                      idx.data_ptr<uint8_t>(), N, H, W, C, Ho, Wo, k, s, p, stream(), is_f32(y));
  return {out, idx};
}

// Its backward: Σg, Σg·x̂ (replica slab `rep`, re-zeroed) -> (+ dγ, dβ accumulators) -> dy.
// Returns (dy, Σg, Σg·x̂).
std::tuple<Tensor, Tensor, Tensor> pool_bn_bwd(Tensor dp, Tensor idx, Tensor pout, Tensor y,
                                               Tensor mean, Tensor invstd, Tensor gamma, Tensor rep,
                                               int64_t count, int k, int s, int p,
                                               optional<Tensor> dgamma, optional<Tensor> dbeta) {
  check_act(dp, "dp");
  check_same(pout, dp, "pout");
  check_same(y, dp, "y");
  check_cuda(idx, "idx");
  c10::DeviceGuard g(dp.device());
  int N = y.size(0), H = y.size(1), W = y.size(2), C = y.size(3);
  int Ho = dp.size(1), Wo = dp.size(2);
  TORCH_CHECK(C % 8 == 0 && 256 % (C / 8) == 0, "pool_bn: C % 8 == 0, 256 % (C/8) == 0");
  TORCH_CHECK(idx.sizes() == dp.sizes() && pout.sizes() == dp.sizes() && dp.size(3) == C,
              "pool_bn_bwd shape mismatch");
  TORCH_CHECK(Ho == pool_out(H, k, s, p, false) && Wo == pool_out(W, k, s, p, false),
              "pool_bn_bwd geometry mismatch");
  for (const Tensor* t : {&mean, &invstd, &gamma}) check_vec(*t, C, "BN vector");
  for (const Tensor* t : {&mean, &invstd})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "pool_bn vectors: 16-B aligned");
  check_f32(rep, "rep");
  TORCH_CHECK(rep.numel() == 3ll * mipipe::kStatReplicas * C, "rep must be [3,R,C]");
  TORCH_CHECK(dgamma.has_value() == dbeta.has_value(), "pass both accumulators or none");
  const bool f32 = is_f32(dp);
  const long pixels = (long)N * H * W;
  if (mipipe::g_deterministic) {
    const int G = mipipe::pool_bn_bwd_reduce_blocks(pixels, C);
    auto part = torch::empty({2, G, C}, dp.options().dtype(at::kFloat));
    float* p0 = part.data_ptr<float>();
    mipipe::pool_bn_bwd_reduce(dp.data_ptr(), idx.data_ptr<uint8_t>(), pout.data_ptr(), y.data_ptr(),
                               mean.data_ptr<float>(), invstd.data_ptr<float>(), N, H, W, C, Ho, Wo,
                               k, s, p, p0, G, stream(), f32);
    // the G rows collected in det_sum_rows' order by one launch (rep stays zero)
    auto o = rep.options();
    auto sg = torch::empty({C}, o), sgx = torch::empty({C}, o);
    mipipe::bn_bwd_collect_rows(p0, G, C, false, sg.data_ptr<float>(), sgx.data_ptr<float>(),
                                nullptr, fptr(dgamma, C), fptr(dbeta, C), nullptr, nullptr, nullptr,
                                stream());
    auto dy = torch::empty_like(y);
    mipipe::pool_bn_bwd_apply(dp.data_ptr(), idx.data_ptr<uint8_t>(), pout.data_ptr(), y.data_ptr(),
                              mean.data_ptr<float>(), invstd.data_ptr<float>(),
                              gamma.data_ptr<float>(), sg.data_ptr<float>(), sgx.data_ptr<float>(),
                              count, dy.data_ptr(), N, H, W, C, Ho, Wo, k, s, p, stream(), f32);
    return {dy, sg, sgx};
  } else {
    mipipe::pool_bn_bwd_reduce(dp.data_ptr(), idx.data_ptr<uint8_t>(), pout.data_ptr(), y.data_ptr(),
                               mean.data_ptr<float>(), invstd.data_ptr<float>(), N, H, W, C, Ho, Wo,
                               k, s, p, rep.data_ptr<float>(), 0, stream(), f32);
  }
  auto o = rep.options();
  auto sg = torch::empty({C}, o), sgx = torch::empty({C}, o);
  mipipe::bn_bwd_collect(rep.data_ptr<float>(), C, sg.data_ptr<float>(), sgx.data_ptr<float>(),
                         fptr(dgamma, C), fptr(dbeta, C), stream());
  auto dy = torch::empty_like(y);
  mipipe::pool_bn_bwd_apply(dp.data_ptr(), idx.data_ptr<uint8_t>(), pout.data_ptr(), y.data_ptr(),
                            mean.data_ptr<float>(), invstd.data_ptr<float>(),
                            gamma.data_ptr<float>(), sg.data_ptr<float>(), sgx.data_ptr<float>(),
                            count, dy.data_ptr(), N, H, W, C, Ho, Wo, k, s, p, stream(), f32);
  return {dy, sg, sgx};
}

// ---- recompute-fused ResNet stem (stem.hip): packed input xp [N][Hp][115][8] bf16, packed
// weights [64][7][4][8] bf16; the 7x7/2 conv output is never stored.
struct StemGeo {
  int N, Ho, Hp;
};
static bool stem_geo_ok(const Tensor& xp, const Tensor& w, StemGeo* g) {
  if (xp.dim() != 4 || xp.size(3) != 8 || w.dim() != 4 || w.size(0) != 64 || w.size(1) != 7 ||
      w.size(2) != 4 || w.size(3) != 8)
    return false;
  const int N = (int)xp.size(0), Hp = (int)xp.size(1), Wsp = (int)xp.size(2);
  const int Ho = (Hp - 7) / 2 + 1, Wo = Wsp - 3;
  if (g != nullptr) *g = StemGeo{N, Ho, Hp};
  return (Hp - 7) % 2 == 0 && mipipe::stem_fused_supported(N, Ho, Wo, Hp, Wsp, 64, Ho / 2, Wo / 2);
}
static StemGeo stem_check(const Tensor& xp, const Tensor& w) {
  check_bf16(xp, "xp");
  check_bf16(w, "w");
  StemGeo g;
  TORCH_CHECK(stem_geo_ok(xp, w, &g), "fused stem: needs xp [N][2*Ho+5][115][8] (112 output "
              "columns, Ho % 4 == 0) and w [64][7][4][8]");
  return g;
}

bool stem_fused_supported(Tensor xp, Tensor w) {
  return xp.is_cuda() && xp.scalar_type() == at::kBFloat16 && w.scalar_type() == at::kBFloat16 &&
         stem_geo_ok(xp, w, nullptr);
}

// Σ(y-shift), Σ(y-shift)² into the zeroed fwd replica slabs [R][64] (re-zeroed by bn_finalize).
std::tuple<Tensor, Tensor> stem_fwd_stats(Tensor xp, Tensor w, Tensor shift, Tensor slab_sum,
                                          Tensor slab_sq) {
  const StemGeo g = stem_check(xp, w);
  c10::DeviceGuard dg(xp.device());
  check_vec(shift, 64, "shift");
  const int R = mipipe::kStatReplicas;
  check_f32(slab_sum, "slab_sum");
  check_f32(slab_sq, "slab_sq");
  TORCH_CHECK(slab_sum.numel() == R * 64 && slab_sq.numel() == R * 64, "stat slabs must be [R, 64]");
  float *s0 = slab_sum.data_ptr<float>(), *s1 = slab_sq.data_ptr<float>();
  if (mipipe::g_deterministic) {
    const int G = mipipe::stem_stats_blocks(g.N, g.Ho);
    auto part = torch::empty({2, G, 64}, xp.options().dtype(at::kFloat));
    float* p0 = part.data_ptr<float>();
    mipipe::stem_fwd_stats(xp.data_ptr(), w.data_ptr(), g.N, g.Ho, g.Hp, shift.data_ptr<float>(), p0,
                           p0 + (long)G * 64, R, G, stream());
    // the partial rows go to bn_finalize (det_sum_rows' order there); the slabs stay zero
    return {part[0], part[1]};
  } else {
    mipipe::stem_fwd_stats(xp.data_ptr(), w.data_ptr(), g.N, g.Ho, g.Hp, shift.data_ptr<float>(), s0,
                           s1, R, 0, stream());
  }
  return {slab_sum, slab_sq};
}

// (maxpool_3x3/2/1(relu(bn(conv(xp)))), window tap (0xFF where the output is not > 0), y)
std::tuple<Tensor, Tensor, optional<Tensor>> stem_fwd_pool(Tensor xp, Tensor w, Tensor scale,
                                                           Tensor bias, bool want_y) {
  const StemGeo g = stem_check(xp, w);
  c10::DeviceGuard dg(xp.device());
  check_vec(scale, 64, "scale");
  check_vec(bias, 64, "bias");
  auto out = torch::empty({g.N, g.Ho / 2, 56, 64}, xp.options());
  auto idx = torch::empty({g.N, g.Ho / 2, 56, 64}, xp.options().dtype(at::kByte));
  optional<Tensor> y;
  if (want_y) y = torch::empty({g.N, g.Ho, 112, 64}, xp.options());
  mipipe::stem_fwd_pool(xp.data_ptr(), w.data_ptr(), g.N, g.Ho, g.Hp, scale.data_ptr<float>(),
                        bias.data_ptr<float>(), out.data_ptr(), idx.data_ptr<uint8_t>(),
                        want_y ? y->data_ptr() : nullptr, stream());
  return {out, idx, y};
}

// Backward of the fused stem: Σg, Σg·x̂ (bwd slab `rep` [3][R][64], re-zeroed; + dγ / dβ
// accumulators) -> packed dW [64][7][4][8] fp32 with the BN-apply folded into the weight-grad.
// Returns (dW, Σg, Σg·x̂).
// The BN-backward statistics come from the POOLED tensors: Σg = Σ_p dp·[z>0] and
// Σg·x̂ = Σ_p dp·[z>0]·(z-β)/γ, z the stored pooled output (= relu(γ·x̂ + β) at the window's
// argmax pixel) — a reduce over 2 x 103 MB (bn_act_bwd_reduce with mean = β, invstd = 1, the
// division by γ in its collect) instead of routing dp to the 411 MB conv output y (143 us).
std::tuple<Tensor, Tensor, Tensor> stem_bwd(Tensor xp, Tensor y, Tensor dp, Tensor idx, Tensor pout,
                                            Tensor mean, Tensor invstd, Tensor gamma, Tensor beta,
                                            Tensor rep, int64_t count, optional<Tensor> dgamma,
                                            optional<Tensor> dbeta) {
  check_bf16(xp, "xp");
  c10::DeviceGuard dg(xp.device());
  const int N = (int)xp.size(0), Hp = (int)xp.size(1), Ho = (Hp - 7) / 2 + 1;
  TORCH_CHECK(xp.dim() == 4 && xp.size(2) == 115 && xp.size(3) == 8 && (Hp - 7) % 2 == 0 &&
                  mipipe::stem_fused_supported(N, Ho, 112, Hp, 115, 64, Ho / 2, 56),
              "stem_bwd: xp must be the packed 224-px stem input");
  check_bf16(y, "y");
  check_bf16(dp, "dp");
  check_bf16(pout, "pout");
  check_cuda(idx, "idx");
  const std::vector<int64_t> ps = {N, Ho / 2, 56, 64}, ys = {N, Ho, 112, 64};
  TORCH_CHECK(dp.sizes() == ps && idx.sizes() == ps && pout.sizes() == ps && y.sizes() == ys &&
                  idx.scalar_type() == at::kByte && dp.is_contiguous() && pout.is_contiguous(),
              "stem_bwd: shape mismatch");
  for (const Tensor* t : {&mean, &invstd, &gamma, &beta}) check_vec(*t, 64, "BN vector");
  check_f32(rep, "rep");
  const int R = mipipe::kStatReplicas;
  TORCH_CHECK(rep.numel() == 3ll * R * 64, "rep must be [3,R,64]");
  TORCH_CHECK(dgamma.has_value() == dbeta.has_value(), "pass both accumulators or none");
  float* r = rep.data_ptr<float>();
  const long pooled = (long)N * (Ho / 2) * 56;
  auto o = rep.options();
  auto sg = torch::empty({64}, o), sgx = torch::empty({64}, o);
  optional<Tensor> det_ws;
  if (mipipe::g_deterministic)
    det_ws = torch::empty({3, (int64_t)mipipe::bn_bwd_reduce_blocks(pooled, 64), 64}, o);
  mipipe::bn_act_bwd_reduce(dp.data_ptr(), pout.data_ptr(), pout.data_ptr(),
                            beta.data_ptr<float>(), nullptr, nullptr, nullptr, nullptr, true,
                            pooled, 64, sg.data_ptr<float>(), sgx.data_ptr<float>(), nullptr, r,
                            fptr(dgamma, 64), fptr(dbeta, 64), nullptr, nullptr, stream(), false,
                            det_ws.has_value() ? det_ws->data_ptr<float>() : nullptr,
                            gamma.data_ptr<float>());
  const int G2 = mipipe::stem_wgrad_blocks(N, Ho);
  auto ws = torch::empty({(int64_t)G2 * 64 * 224}, o);
  auto dw = torch::zeros({64, 7, 4, 8}, o);
  mipipe::stem_bwd_wgrad(xp.data_ptr(), y.data_ptr(), N, Ho, Hp, dp.data_ptr(),
                         idx.data_ptr<uint8_t>(), mean.data_ptr<float>(), invstd.data_ptr<float>(),
                         gamma.data_ptr<float>(), sg.data_ptr<float>(), sgx.data_ptr<float>(), count,
                         ws.data_ptr<float>(), dw.data_ptr<float>(), stream());
  return {dw, sg, sgx};
}

Tensor maxpool_bwd(Tensor dy, Tensor idx, std::vector<int64_t> xs, int k, int s, int p) {
  check_act(dy, "dy");
  check_cuda(idx, "idx");
  c10::DeviceGuard g(dy.device());
  TORCH_CHECK(xs.size() == 4 && dy.dim() == 4, "maxpool_bwd: NHWC shapes expected");
  int N = xs[0], H = xs[1], W = xs[2], C = xs[3];
  int Ho = dy.size(1), Wo = dy.size(2);
  TORCH_CHECK(C % 8 == 0 && k <= 15, "maxpool needs C % 8 == 0 and k <= 15");
  TORCH_CHECK(k >= 1 && s >= 1 && p >= 0 && 2 * p <= k, "bad maxpool geometry");
  TORCH_CHECK(idx.scalar_type() == at::kByte && idx.sizes() == dy.sizes() && dy.size(3) == C,
              "maxpool_bwd shape mismatch");
  TORCH_CHECK(dy.size(0) == N, "maxpool_bwd: dy batch ", dy.size(0), " != x batch ", N);
  // the forward's extent: floor, or ceil when it ran in ceil mode
  TORCH_CHECK((Ho == pool_out(H, k, s, p, false) || Ho == pool_out(H, k, s, p, true)) &&
                  (Wo == pool_out(W, k, s, p, false) || Wo == pool_out(W, k, s, p, true)),
              "maxpool_bwd: dy extent ", Ho, " x ", Wo, " does not match the pooling geometry");
  auto dx = torch::empty({N, H, W, C}, dy.options());
  mipipe::maxpool_bwd(dy.data_ptr(), idx.data_ptr<uint8_t>(), dx.data_ptr(), N, H, W, C, Ho, Wo, k,
                      s, p, stream(), is_f32(dy));
  return dx;
}

Tensor avgpool_fwd(Tensor x) {
  check_act(x, "x");
  c10::DeviceGuard g(x.device());
  int N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
  TORCH_CHECK(C % 8 == 0, "avgpool needs C % 8 == 0");
  auto y = torch::empty({N, C}, x.options());
  mipipe::avgpool_fwd(x.data_ptr(), y.data_ptr(), N, HW, C, stream(), is_f32(x));
  return y;
}

Tensor avgpool_bwd(Tensor dy, std::vector<int64_t> xs) {
  check_act(dy, "dy");
  c10::DeviceGuard g(dy.device());
  int N = xs[0], H = xs[1], W = xs[2], C = xs[3];
  TORCH_CHECK(dy.size(0) == N && dy.size(1) == C, "avgpool_bwd shape mismatch");
  auto dx = torch::empty({N, H, W, C}, dy.options());
  mipipe::avgpool_bwd(dy.data_ptr(), dx.data_ptr(), N, H * W, C, stream(), is_f32(dy));
  return dx;
}

// ------------------------------------------------------------------------------- GEMM
// WsFinish tickets (launchers.hpp): one zeroed int array per device, handed out as a ring of
// per-call slices.  Every launch leaves its slice zeroed again (the last split of a tile resets
// its ticket), so a slice is reusable as soon as its kernel completed; a graph replays the
// slices it captured.  Created eagerly (never inside a stream capture: the zero-fill would be
// captured and the buffer would live in the graph's pool) — before that, plans fall back to the
// separate slice sum.
namespace {
struct TicketRing {
  Tensor buf;
  long next = 0;
};
std::unordered_map<int, TicketRing> g_ticket_rings;
constexpr long kTicketCap = 1 << 20;

// Opt-in (MIPIPE_WS_FINISH=1): measured SLOWER on BERT-base — 4,125 vs 4,384 seq/s, GEMM time
// 5.27 vs 4.74 ms/step with the sum kernels (profiles/r4_ws_finish_experiment.txt).  The
// agent-scope release / acquire fences around the ticket are an L2 write-back and an L2
// INVALIDATE of the whole XCD (buffer_wbl2 / buffer_inv sc1): every block that finishes a split
// throws away the operand tiles its neighbours on that XCD were reusing.
bool g_ws_finish = env_flag("MIPIPE_WS_FINISH", false);

int* ws_tickets(const Tensor& like, long n) {
  if (!g_ws_finish || n <= 0 || n > kTicketCap) return nullptr;
  TicketRing& r = g_ticket_rings[like.get_device()];
  if (!r.buf.defined()) {
    if (tune::capturing()) return nullptr;
    r.buf = torch::zeros({kTicketCap}, like.options().dtype(at::kInt));
  }
  if (r.next + n > kTicketCap) r.next = 0;
  int* p = r.buf.data_ptr<int>() + r.next;
  r.next = (r.next + n + 63) & ~63l;
  return p;
}
}  // namespace

Tensor gemm(Tensor a, Tensor b, bool trans_a, bool trans_b, optional<Tensor> bias,
            std::string act, at::ScalarType out_dtype, optional<Tensor> c, double beta,
            int64_t plan, optional<Tensor> addend, optional<std::vector<Tensor>> prefetch) {
  check_act(a, "A");
  check_same(b, a, "B");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "gemm expects 2-D operands");
  int64_t M = trans_a ? a.size(1) : a.size(0);
  int64_t K = trans_a ? a.size(0) : a.size(1);
  int64_t N = trans_b ? b.size(0) : b.size(1);
  int64_t Kb = trans_b ? b.size(1) : b.size(0);
  TORCH_CHECK(K == Kb, "gemm inner dims differ: ", K, " vs ", Kb);
  TORCH_CHECK(M % 8 == 0 || !trans_a, "A^T operand needs M % 8 == 0");
  TORCH_CHECK(K % 8 == 0 || (trans_a && !trans_b), "K-contiguous operands need K % 8 == 0");
  TORCH_CHECK(N % 8 == 0, "gemm needs N % 8 == 0, got ", N);
  TORCH_CHECK(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "gemm dims too large");
  int act_i = act == "relu" ? 1 : 0;
  TORCH_CHECK(act == "none" || act == "relu", "gemm epilogue act must be none|relu");
  const float* bias_p = nullptr;
  if (bias.has_value()) {
    check_vec(*bias, N, "bias");
    bias_p = bias->data_ptr<float>();
  }
  Tensor out;
  int mode;
  if (c.has_value() && beta != 0.0) {
    TORCH_CHECK(beta == 1.0, "gemm supports beta in {0, 1}");
    check_f32(*c, "C");
    TORCH_CHECK(c->size(0) == M && c->size(1) == N, "C shape mismatch");
    TORCH_CHECK(c->stride(1) == 1 && c->stride(0) == N, "accumulated C must be contiguous");
    TORCH_CHECK(bias_p == nullptr && act_i == 0, "accumulating gemm has no epilogue");
    out = *c;
    mode = 2;
  } else if (out_dtype == a.scalar_type()) {  // activation dtype: bias / ReLU epilogue
    out = torch::empty({M, N}, a.options());
    mode = 0;
  } else {
    TORCH_CHECK(out_dtype == at::kFloat, "gemm out dtype must be the operand dtype or fp32");
    out = torch::empty({M, N}, a.options().dtype(at::kFloat));
    mode = 1;
    TORCH_CHECK(act_i == 0, "fp32 gemm output has no activation epilogue");
  }
  const bool f32 = is_f32(a);
  // bf16 operands go through buffer descriptors with 32-bit byte offsets (gemm_core.hpp kOOB)
  TORCH_CHECK(f32 || ((trans_a ? K : M) * a.stride(0) * 2 < (1ll << 31) - (1ll << 24) &&
                      (trans_b ? N : K) * b.stride(0) * 2 < (1ll << 31) - (1ll << 24)),
              "bf16 gemm operands beyond 2 GiB are not supported");
  const void* add_p = nullptr;
  if (addend.has_value()) {
    TORCH_CHECK(mode == 0 && !trans_a && !trans_b && bias_p == nullptr && act_i == 0,
                "gemm addend: activation-dtype output of A[M][K] @ B[K][N], no bias / act");
    check_same(*addend, a, "addend");
    TORCH_CHECK(addend->dim() == 2 && addend->size(0) == M && addend->size(1) == N &&
                addend->is_contiguous(), "addend must be a contiguous [M, N] tensor");
    add_p = addend->data_ptr();
  }
  // Workspace split-K: each split stores its partial tile into its own fp32 slice with plain
  // stores (no atomics: deterministic), then one pass sums the slices in order —
  //  * accumulating GEMMs (weight-grads into the flat fp32 gradient, mode 2): splitk_sum adds
  //    them to C.  Chosen by the tuner where the output is small against the CU count (BERT's
  //    768 x 768 / 768 x 3072 weight-grads: 36-144 tiles) and atomics would cost more;
  //  * activation-dtype outputs with at most a bias or an addend (mode 0: the MLM decoder's
  //    data-grad with K = 30528 — 30 output tiles for 256 CUs — or BERT's FFN-out projection,
  //    K = 3072; mode 3: the FFN-in / QKV data-grads with the residual gradient added):
  //    splitk_sum_bf16 adds the slices, the bias / addend and rounds once to bf16.
  // Split counts 2..8 (not only powers of two): tiles x splits can then land near a whole
  // number of waves over the 256 CUs.
  // Plans with Plan::ws set.  (Round 3 also timed a hipBLASLt "library plan" here; it is gone:
  // every GEMM of the training step runs on the MFMA kernels, tools/gemm_plans.py.)
  const bool ws_out0 = mode == 0 && act_i == 0 && N % 8 == 0;
  // another GEMM's cold operands, warmed by this one's blocks (mipipe/ops/prefetch.py)
  mipipe::TouchRanges pf;
  if (prefetch.has_value())
    for (const Tensor& t : *prefetch) {
      if (pf.count == 2) break;
      TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.device() == a.device(),
                  "gemm prefetch: contiguous tensors on the operands' device");
      if (t.numel() == 0) continue;
      pf.ptr[pf.count] = static_cast<const uint8_t*>(t.data_ptr());
      pf.bytes[pf.count++] = (long)(t.numel() * t.element_size());
    }
  const mipipe::TouchRanges* pfp = pf.count > 0 ? &pf : nullptr;
  auto launch = [&](void* C, const mipipe::Plan& p) {
    const int cfg = p.tile, sp = p.splits;
    if (p.ws && (mode == 2 || ws_out0) && sp > 1) {
      const int ns = mipipe::gemm_ws_splits((int)K, sp);
      Tensor ws = torch::empty({(int64_t)ns, M, N}, a.options().dtype(at::kFloat));
      mipipe::WsFinish fin;
      // (an fp32 activation output is finished by the separate ordered sum: ws_finish adds into
      // fp32 targets)
      fin.ticket = ns > 1 && N % 4 == 0 && (mode == 2 || !f32)
                       ? ws_tickets(a, mipipe::gemm_max_tiles(M, N)) : nullptr;
      fin.out = C;
      fin.ldo = N;
      fin.bias = bias_p;
      fin.addend = add_p;
      fin.bf16 = mode == 2 ? 0 : 1;
      mipipe::gemm(a.data_ptr(), a.stride(0), !trans_a, b.data_ptr(), b.stride(0), trans_b,
                   ws.data_ptr(), N, (int)M, (int)N, (int)K, nullptr, 0, 2, stream(), f32, cfg,
                   sp, nullptr, true, fin.ticket != nullptr ? &fin : nullptr, nullptr, pfp);
      if (fin.ticket != nullptr) return;  // the GEMM's last split per tile summed the slices
      if (mode == 2)
        mipipe::splitk_sum(ws.data_ptr<float>(), ns, M * N, static_cast<float*>(C), stream());
      else if (f32)
        mipipe::splitk_sum_f32out(ws.data_ptr<float>(), ns, M, (int)N, bias_p, static_cast<float*>(C),
                                  N, stream(), static_cast<const float*>(add_p));
      else
        mipipe::splitk_sum_bf16(ws.data_ptr<float>(), ns, M, (int)N, bias_p, C, N, stream(),
                                add_p);
      return;
    }
    mipipe::gemm(a.data_ptr(), a.stride(0), !trans_a, b.data_ptr(), b.stride(0), trans_b, C, N,
                 (int)M, (int)N, (int)K, bias_p, act_i, mode, stream(), f32, cfg, sp, add_p,
                 false, nullptr, nullptr, pfp);
  };
  if (plan < 0) {
    std::vector<int> cands = tune::gemm_candidates(f32, mode == 2);
    // (fp32 activation outputs: small grids too — the reference config's fc layer, 64-128 output
    // tiles of 8-16 k-steps)
    const bool small_f32 = ws_out0 && f32 && K >= 256 && ((M + 127) / 128) * ((N + 63) / 64) < 256;
    if ((mode == 2 && K >= 1024) || (ws_out0 && K >= 2048) || small_f32) {
      for (int t : tune::candidates(f32, mode == 2))
        for (int sp : {2, 3, 4, 6, 8}) cands.push_back(mipipe::encode_gemm_plan(t, sp, true));
    }
    plan = tune::select_from(tune::gemm_key(M, N, K, !trans_a, trans_b, add_p != nullptr ? 3 : mode, f32),
                             cands, [&](int p) {
                               auto scratch = mode == 2 ? torch::zeros_like(out)
                                                        : torch::empty_like(out);
                               launch(scratch.data_ptr(), mipipe::decode_gemm_plan(p, true));
                             });
  }
  launch(out.data_ptr(), mipipe::decode_gemm_plan((int)plan, true));
  return out;
}

// GELU Linear forward in one GEMM: (y = gelu(A B^T + bias), h = A B^T + bias), bf16, A [M][K],
// B [N][K] (the nn.Linear layout).  The plan comes from the plain bf16 GEMM's table entry of the
// same shape (same main loop), timed with the GELU epilogue when missing.
std::tuple<Tensor, Tensor> gemm_gelu(Tensor a, Tensor b, optional<Tensor> bias, int64_t plan) {
  check_bf16(a, "A");
  check_same(b, a, "B");
  c10::DeviceGuard g(a.device());
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1), "gemm_gelu shapes");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous(), "gemm_gelu operands must be contiguous");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(N % 8 == 0 && K % 8 == 0 && M < (1ll << 31), "gemm_gelu needs N, K % 8 == 0");
  const float* bias_p = nullptr;
  if (bias.has_value()) {
    check_vec(*bias, N, "bias");
    bias_p = bias->data_ptr<float>();
  }
  auto y = torch::empty({M, N}, a.options()), h = torch::empty({M, N}, a.options());
  auto launch = [&](void* yo, void* ho, const mipipe::Plan& p) {  // (a plain-GEMM plan: its tile)
    mipipe::gemm(a.data_ptr(), K, true, b.data_ptr(), K, true, yo, N, (int)M, (int)N, (int)K,
                 bias_p, 2, 0, stream(), false, p.tile, -1, nullptr, false, nullptr, ho);
  };
  if (plan < 0) {
    plan = tune::select_from(tune::gemm_key(M, N, K, true, true, 0, false),
                             tune::gemm_candidates(false, false), [&](int p) {
                               auto ys = torch::empty_like(y), hs = torch::empty_like(h);
                               launch(ys.data_ptr(), hs.data_ptr(), mipipe::decode_gemm_plan(p, true));
                             });
  }
  launch(y.data_ptr(), h.data_ptr(), mipipe::decode_gemm_plan((int)plan, true));
  return {y, h};
}

// Cache warming of GEMM operands (mipipe/ops/prefetch.py): one load per 64-B line of each
// tensor's bytes on the current stream, nothing written.
void touch(std::vector<Tensor> ts) {
  mipipe::TouchRanges r;
  for (size_t i = 0; i < ts.size(); ++i) {
    const Tensor& t = ts[i];
    TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "touch: contiguous GPU tensors");
    if (t.numel() == 0) continue;
    r.ptr[r.count] = static_cast<const uint8_t*>(t.data_ptr());
    r.bytes[r.count] = (long)(t.numel() * t.element_size());
    if (++r.count == mipipe::kTouchRanges) {
      c10::DeviceGuard g(t.device());
      mipipe::touch(r, stream());
      r.count = 0;
    }
  }
  if (r.count > 0) {
    c10::DeviceGuard g(ts[0].device());
    mipipe::touch(r, stream());
  }
}

// ------------------------------------------------------------------------------- optim
// ---- flat-buffer kernels (csrc/kernels/optim.hip, ema.hip): the argument checks they share
// p and every named state tensor: fp32, contiguous, on the GPU, p's size (a multiple of `align`),
// 16-B aligned.  Returns the size.
struct FlatArg {
  const Tensor& t;
  const char* name;
};
static int64_t flat_n(const Tensor& p, int64_t align, std::initializer_list<FlatArg> state) {
  const int64_t n = p.numel();
  TORCH_CHECK(n % align == 0, "flat buffer size must be a multiple of ", align);
  auto check = [n](const Tensor& t, const char* name) {
    check_f32(t, name);
    TORCH_CHECK(t.numel() == n, name, " size mismatch");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-B aligned");
  };
  check(p, "param");
  for (const FlatArg& a : state) check(a.t, a.name);
  return n;
}

// The bf16 shadow of the flat parameters (optional), written with 8-byte stores.
static void* flat_shadow(const optional<Tensor>& shadow, int64_t n) {
  if (!shadow.has_value()) return nullptr;
  check_cuda(*shadow, "shadow");
  TORCH_CHECK(shadow->numel() == n && shadow->scalar_type() == at::kBFloat16, "shadow mismatch");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(shadow->data_ptr()) % 8 == 0, "shadow must be 8-B aligned");
  return shadow->data_ptr();
}

// A per-step count that lives on the device: int32 [1].
static const int* dev_counter(const Tensor& t, const char* name) {
  check_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kInt && t.numel() == 1, name, " must be int32 [1]");
  return t.data_ptr<int>();
}

void sgd_step(Tensor p, Tensor g, Tensor m, optional<Tensor> shadow, double lr, double momentum,
              double dampening, double wd, bool nesterov, bool first, double grad_scale) {
  const int64_t n = flat_n(p, 4, {{g, "grad"}, {m, "momentum"}});
  c10::DeviceGuard gd(p.device());
  void* sh = flat_shadow(shadow, n);
  mipipe::sgd_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), sh, n, (float)lr,
                   (float)momentum, (float)dampening, (float)wd, nesterov, first,
                   (float)grad_scale, stream());
}

// an optional device word mixed into a dropout seed (the transformer ops below)
static const int* i32_dev(const optional<Tensor>& t, const char* name) {
  if (!t.has_value()) return nullptr;
  check_cuda(*t, name);
  TORCH_CHECK(t->scalar_type() == at::kInt && t->numel() >= 1, name, " must be an int32 device counter");
  return t->data_ptr<int>();
}

void adamw_step(Tensor p, Tensor g, Tensor m, Tensor v, optional<Tensor> shadow, double lr,
                double b1, double b2, double eps, double wd, int64_t step, double grad_scale,
                optional<Tensor> step_dev) {
  const int64_t n = flat_n(p, 4, {{g, "grad"}, {m, "exp_avg"}, {v, "exp_avg_sq"}});
  c10::DeviceGuard gd(p.device());
  void* sh = flat_shadow(shadow, n);
  double bc1 = 1.0 - std::pow(b1, (double)step), bc2 = 1.0 - std::pow(b2, (double)step);
  mipipe::adamw_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                     v.data_ptr<float>(), sh, n, (float)lr, (float)b1, (float)b2, (float)eps,
                     (float)wd, (float)bc1, (float)bc2, (float)grad_scale, stream(),
                     step_dev.has_value() ? dev_counter(*step_dev, "step_dev") : nullptr);
}

// ---- LARS / LAMB (csrc/kernels/optim.hip): the optimizer's device tables, checked per call
struct OptimTabs {
  const int *chunks, *segs;
  int nchunks, nseg;
  float *part, *segtot, *ratio, *scal;
  const int* t_dev;
};
static OptimTabs optim_tabs(const Tensor& chunks, const Tensor& segs, const Tensor& part,
                            const Tensor& segtot, const Tensor& ratio, const Tensor& scal,
                            const Tensor& t_dev) {
  auto i4 = [](const Tensor& t, const char* name) {
    check_cuda(t, name);
    TORCH_CHECK(t.scalar_type() == at::kInt && t.dim() == 2 && t.size(1) == 4, name,
                " must be int32 [n, 4]");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-B aligned");
  };
  i4(chunks, "chunks");
  i4(segs, "segs");
  OptimTabs o;
  o.nchunks = (int)chunks.size(0);
  o.nseg = (int)segs.size(0);
  TORCH_CHECK(o.nseg >= 1 && o.nchunks >= o.nseg, "optimizer tables: every segment has a chunk");
  check_vec(part, 2 * (int64_t)o.nchunks, "part");
  check_vec(segtot, 2 * (int64_t)o.nseg, "segtot");
  check_vec(ratio, o.nseg, "ratio");
  check_vec(scal, 4, "scal");
  o.chunks = chunks.data_ptr<int>();
  o.segs = segs.data_ptr<int>();
  o.part = part.data_ptr<float>();
  o.segtot = segtot.data_ptr<float>();
  o.ratio = ratio.data_ptr<float>();
  o.scal = scal.data_ptr<float>();
  o.t_dev = dev_counter(t_dev, "step_dev");
  return o;
}

static mipipe::OptimSched optim_sched(int64_t kind, double base, double end, int64_t warmup,
                                      int64_t total) {
  TORCH_CHECK(kind >= 0 && kind <= 3, "schedule kind must be 0..3");
  TORCH_CHECK(warmup >= 0 && total >= 0 && warmup < (1ll << 31) && total < (1ll << 31),
              "schedule steps out of range");
  return mipipe::OptimSched{(int)kind, (float)base, (float)end, (int)warmup, (int)total};
}

// One LARS step (3 launches; 2 when neither the trust ratio nor clipping needs the norms).
// tc < 0: no trust ratio.  max_norm <= 0: no clipping.
void lars_step(Tensor p, Tensor g, Tensor m, optional<Tensor> shadow, Tensor chunks, Tensor segs,
               Tensor part, Tensor segtot, Tensor ratio, Tensor scal, Tensor step_dev,
               double momentum, double tc, double eps, double max_norm, double grad_scale,
               int64_t kind, double base_lr, double end_lr, int64_t warmup, int64_t total) {
  const int64_t n = flat_n(p, 64, {{g, "grad"}, {m, "momentum"}});
  c10::DeviceGuard gd(p.device());
  void* sh = flat_shadow(shadow, n);
  const OptimTabs t = optim_tabs(chunks, segs, part, segtot, ratio, scal, step_dev);
  const auto sc = optim_sched(kind, base_lr, end_lr, warmup, total);
  const bool norms = tc >= 0 || max_norm > 0;
  if (norms)
    mipipe::optim_seg_sumsq(p.data_ptr<float>(), g.data_ptr<float>(), t.chunks, t.nchunks, t.nseg,
                            n, (float)grad_scale, true, t.part, stream());
  mipipe::optim_seg_finish(t.part, t.nchunks, t.segs, t.nseg, t.segtot, t.ratio, t.scal, t.t_dev,
                           norms ? 0 : 3, (float)tc, (float)eps, (float)max_norm, sc, stream());
  mipipe::optim_lars_apply(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), sh,
                           t.chunks, t.segs, t.nchunks, t.nseg, n, (float)grad_scale,
                           (float)momentum, t.ratio, t.scal, stream());
}

// One LAMB step: moments, finish, apply; with max_norm > 0 a gradient-norm pass and its finish
// come first (5 launches).
void lamb_step(Tensor p, Tensor g, Tensor m, Tensor v, optional<Tensor> shadow, Tensor chunks,
               Tensor segs, Tensor part, Tensor segtot, Tensor ratio, Tensor scal,
               Tensor step_dev, double b1, double b2, double eps, double max_norm,
               double grad_scale, int64_t kind, double base_lr, double end_lr, int64_t warmup,
               int64_t total) {
  TORCH_CHECK(b1 > 0 && b1 < 1 && b2 > 0 && b2 < 1, "LAMB betas must lie in (0, 1)");
  const int64_t n = flat_n(p, 64, {{g, "grad"}, {m, "exp_avg"}, {v, "exp_avg_sq"}});
  c10::DeviceGuard gd(p.device());
  void* sh = flat_shadow(shadow, n);
  const OptimTabs t = optim_tabs(chunks, segs, part, segtot, ratio, scal, step_dev);
  const auto sc = optim_sched(kind, base_lr, end_lr, warmup, total);
  float *pp = p.data_ptr<float>(), *gp = g.data_ptr<float>();
  float *mp = m.data_ptr<float>(), *vp = v.data_ptr<float>();
  const float lnb1 = (float)std::log(b1), lnb2 = (float)std::log(b2);
  if (max_norm > 0) {
    mipipe::optim_seg_sumsq(pp, gp, t.chunks, t.nchunks, t.nseg, n, (float)grad_scale, false,
                            t.part, stream());
    mipipe::optim_seg_finish(t.part, t.nchunks, t.segs, t.nseg, t.segtot, t.ratio, t.scal, t.t_dev,
                             1, 0.f, 0.f, (float)max_norm, sc, stream());
  }
  mipipe::optim_lamb_moments(pp, gp, mp, vp, t.chunks, t.segs, t.nchunks, t.nseg, n,
                             (float)grad_scale, (float)b1, (float)(1.0 - b1), (float)b2,
                             (float)(1.0 - b2), lnb1, lnb2, (float)eps,
                             max_norm > 0 ? t.scal : nullptr, t.t_dev, t.part,
                             stream());
  mipipe::optim_seg_finish(t.part, t.nchunks, t.segs, t.nseg, t.segtot, t.ratio, t.scal, t.t_dev, 2,
                           0.f, 0.f, 0.f, sc, stream());
  mipipe::optim_lamb_apply(pp, mp, vp, sh, t.chunks, t.segs, t.nchunks, t.nseg, n, lnb1, lnb2,
                           (float)eps, t.ratio, t.scal, t.t_dev, stream());
}

// ---- weight EMA (csrc/kernels/ema.hip)
static const int* check_ema_args(const Tensor& t_dev, int64_t every, double w_min) {
  const int* t = dev_counter(t_dev, "calls_dev");
  TORCH_CHECK(every >= 1 && every < (1ll << 31), "every must be >= 1");
  TORCH_CHECK(w_min >= 0 && w_min <= 1, "w_min = 1 - decay must lie in [0, 1]");
  return t;
}

// One call of the parameter average: e += w (p - e) when calls_dev % every == 0, else nothing.
void ema_update(Tensor p, Tensor e, Tensor t_dev, int64_t every, double w_min, bool warmup,
                Tensor scal) {
  const int64_t n = flat_n(p, 64, {{e, "ema"}});
  TORCH_CHECK(p.data_ptr() != e.data_ptr(), "ema must not alias param");
  const int* t = check_ema_args(t_dev, every, w_min);
  check_f32(scal, "scal");
  TORCH_CHECK(scal.numel() >= 1, "scal must hold one float");
  c10::DeviceGuard gd(p.device());
  mipipe::ema_update(p.data_ptr<float>(), e.data_ptr<float>(), n, t,
                     (int)every, (float)w_min, warmup, scal.data_ptr<float>(), stream());
}

void ema_swap(Tensor p, Tensor e, optional<Tensor> shadow) {
  const int64_t n = flat_n(p, 64, {{e, "ema"}});
  TORCH_CHECK(p.data_ptr() != e.data_ptr(), "ema must not alias param");
  c10::DeviceGuard gd(p.device());
  void* sh = flat_shadow(shadow, n);
  mipipe::ema_swap(p.data_ptr<float>(), e.data_ptr<float>(), sh, n, stream());
}

static int ema_table_rows(const Tensor& table, const Tensor& eb) {
  check_cuda(table, "table");
  TORCH_CHECK(table.scalar_type() == at::kLong && table.dim() == 2 && table.size(1) == 3,
              "table must be int64 [rows, 3]");
  check_f32(eb, "ema buffers");
  TORCH_CHECK(table.size(0) < (1ll << 31), "too many table rows");
  return (int)table.size(0);
}

void ema_buffers_update(Tensor table, Tensor eb, Tensor t_dev, int64_t every, double w_min,
                        bool warmup) {
  const int rows = ema_table_rows(table, eb);
  const int* t = check_ema_args(t_dev, every, w_min);
  c10::DeviceGuard gd(eb.device());
  mipipe::ema_buffers_update((const long*)table.data_ptr<int64_t>(), rows, eb.data_ptr<float>(),
                             eb.numel(), t, (int)every, (float)w_min, warmup, stream());
}

void ema_buffers_swap(Tensor table, Tensor eb) {
  const int rows = ema_table_rows(table, eb);
  c10::DeviceGuard gd(eb.device());
  mipipe::ema_buffers_swap((const long*)table.data_ptr<int64_t>(), rows, eb.data_ptr<float>(),
                           eb.numel(), stream());
}

// ------------------------------------------------------------------------------- transformer ops
Tensor gelu_fwd(Tensor x) {
  check_bf16(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.numel() % 8 == 0, "gelu needs numel % 8 == 0");
  auto y = torch::empty_like(x);
  mipipe::gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), stream());
  return y;
}

Tensor gelu_bwd(Tensor dy, Tensor x) {
  check_bf16(dy, "dy");
  check_bf16(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.sizes() == dy.sizes() && x.numel() % 8 == 0, "gelu_bwd shape mismatch");
  auto dx = torch::empty_like(x);
  mipipe::gelu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), stream());
  return dx;
}

// dx = gelu_bwd(dy, x) and bias += Σ_rows dx (fp32 [cols], e.g. the flat-gradient view) in one
// kernel; bias sums the bf16-rounded dx (fixed order in deterministic mode).
Tensor gelu_bwd_colsum(Tensor dy, Tensor x, Tensor bias) {
  check_bf16(dy, "dy");
  check_bf16(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.sizes() == dy.sizes() && x.is_contiguous() && dy.is_contiguous(),
              "gelu_bwd_colsum shape mismatch");
  int64_t cols = x.size(-1), rows = x.numel() / cols;
  TORCH_CHECK(cols % 8 == 0, "gelu_bwd_colsum needs cols % 8 == 0");
  check_vec(bias, cols, "bias");
  auto dx = torch::empty_like(x);
  optional<Tensor> work;
  if (mipipe::g_deterministic)
    work = torch::empty({(int64_t)mipipe::gelu_bwd_colsum_blocks(rows, (int)cols), cols},
                        x.options().dtype(at::kFloat));
  mipipe::gelu_bwd_colsum(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), bias.data_ptr<float>(), rows,
                          (int)cols, work.has_value() ? work->data_ptr<float>() : nullptr,
                          stream());
  return dx;
}

std::tuple<Tensor, Tensor, Tensor, optional<Tensor>> layernorm_fwd(Tensor x, Tensor gamma,
                                                                   Tensor beta, double eps,
                                                                   optional<Tensor> res,
                                                                   double drop_p, int64_t drop_seed,
                                                                   optional<Tensor> drop_seed_dev) {
  check_bf16(x, "x");
  c10::DeviceGuard g(x.device());
  int64_t H = x.size(-1), rows = x.numel() / H;
  TORCH_CHECK(H % 8 == 0 && H <= 2048, "layernorm needs H % 8 == 0 and H <= 2048");
  check_vec(gamma, H, "gamma");
  check_vec(beta, H, "beta");
  optional<Tensor> xs;
  if (res.has_value()) {
    check_bf16(*res, "residual");
    TORCH_CHECK(res->sizes() == x.sizes(), "residual shape mismatch");
    xs = torch::empty_like(x);
  }
  auto y = torch::empty_like(x);
  auto o = x.options().dtype(at::kFloat);
  auto shp = x.sizes().vec();
  shp.pop_back();
  auto mean = torch::empty(shp, o), rstd = torch::empty(shp, o);
  TORCH_CHECK(drop_p >= 0.0 && drop_p < 1.0, "dropout p must be in [0, 1)");
  TORCH_CHECK(drop_p == 0.0 || res.has_value(), "fused dropout needs the residual (xsum is saved)");
  const mipipe::DropSpec ds{(float)drop_p, (uint32_t)drop_seed,
                            (const uint32_t*)i32_dev(drop_seed_dev, "drop_seed_dev")};
  mipipe::layernorm_fwd(x.data_ptr(), ptr_or_null(res), gamma.data_ptr<float>(),
                        beta.data_ptr<float>(), y.data_ptr(), xs.has_value() ? xs->data_ptr() : nullptr,
                        mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, (int)H, (float)eps,
                        stream(), drop_p > 0.0 ? &ds : nullptr);
  return {y, mean, rstd, xs};
}

std::tuple<Tensor, optional<Tensor>, optional<Tensor>, optional<Tensor>> layernorm_bwd(
    Tensor dy, Tensor x, Tensor mean, Tensor rstd, Tensor gamma, optional<Tensor> dgamma_acc,
    optional<Tensor> dbeta_acc, double drop_p, int64_t drop_seed,
    optional<Tensor> drop_seed_dev, optional<Tensor> dbias_acc, optional<Tensor> dsum) {
  check_bf16(dy, "dy");
  check_bf16(x, "x");
  c10::DeviceGuard g(x.device());
  int64_t H = x.size(-1), rows = x.numel() / H;
  TORCH_CHECK(H % 8 == 0 && H <= 2048 && dy.sizes() == x.sizes(), "layernorm_bwd shape mismatch");
  check_vec(gamma, H, "gamma");
  TORCH_CHECK(mean.numel() == rows && rstd.numel() == rows, "mean/rstd size mismatch");
  TORCH_CHECK(dgamma_acc.has_value() == dbeta_acc.has_value(), "pass both accumulators or none");
  auto dx = torch::empty_like(x);
  auto o = x.options().dtype(at::kFloat);
  optional<Tensor> dg, db;
  float *pg, *pb;
  if (dgamma_acc.has_value()) {
    pg = fptr(dgamma_acc, H);
    pb = fptr(dbeta_acc, H);
  } else {
    dg = torch::zeros({H}, o);
    db = torch::zeros({H}, o);
    pg = dg->data_ptr<float>();
    pb = db->data_ptr<float>();
  }
  // dbias_acc: also += Σ_rows of the branch gradient (dxd, else dx) — the bias gradient of the
  // Linear that produced x (fp32 [H], e.g. its flat-gradient view)
  float* pd = dbias_acc.has_value() ? fptr(dbias_acc, H) : nullptr;
  auto work = torch::empty({(pd ? 3 : 2) * (int64_t)mipipe::layernorm_bwd_blocks(rows), H}, o);
  TORCH_CHECK(drop_p >= 0.0 && drop_p < 1.0, "dropout p must be in [0, 1)");
  optional<Tensor> dxd;
  const mipipe::DropSpec ds{(float)drop_p, (uint32_t)drop_seed,
                            (const uint32_t*)i32_dev(drop_seed_dev, "drop_seed_dev")};
  if (drop_p > 0.0) dxd = torch::empty_like(x);
  // dsum: the residual stream's gradient (pre-LN blocks), added to dx before its one rounding
  if (dsum.has_value()) {
    check_bf16(*dsum, "dsum");
    TORCH_CHECK(dsum->sizes() == x.sizes() && dsum->device() == x.device(),
                "dsum must have dx's shape and device");
    TORCH_CHECK(drop_p == 0.0, "layernorm_bwd: dsum is not combined with the fused dropout");
  }
  mipipe::layernorm_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                        gamma.data_ptr<float>(), dx.data_ptr(), pg, pb, work.data_ptr<float>(),
                        rows, (int)H, stream(), dxd.has_value() ? dxd->data_ptr() : nullptr,
                        drop_p > 0.0 ? &ds : nullptr, pd, ptr_or_null(dsum));
  return {dx, dg, db, dxd};
}

// ordered (or deterministic mode): no float atomics — large tables through a stable sort of the
// ids and one writer per row (embedding_bwd_sorted), small tables through per-block partial
// tables summed in block order.  scale multiplies the scattered rows (ordered path only).
// sorted_ids / perm: a stable sort of idx computed ahead (DDP sorts the world's ids during the
// forward); ids may then be negative (padding rows: skipped).
Tensor embedding_bwd(Tensor dy, Tensor idx, int64_t num_rows, optional<Tensor> out, bool ordered,
                     double scale, optional<Tensor> sorted_ids, optional<Tensor> perm) {
  check_bf16(dy, "dy");
  check_cuda(idx, "idx");
  c10::DeviceGuard g(dy.device());
  int64_t H = dy.size(-1), n = dy.numel() / H;
  TORCH_CHECK(idx.numel() == n && idx.scalar_type() == at::kLong, "embedding_bwd idx mismatch");
  TORCH_CHECK(H % 8 == 0 && H <= 2048, "embedding_bwd needs H % 8 == 0, H <= 2048");
  TORCH_CHECK(sorted_ids.has_value() == perm.has_value(), "embedding_bwd: sorted_ids with perm");
  Tensor o;
  if (out.has_value()) {  // accumulate into (e.g. the flat-gradient view of the table)
    check_f32(*out, "out");
    TORCH_CHECK(out->is_contiguous() && out->numel() == num_rows * H, "out must be [rows, H]");
    o = *out;
  } else {
    o = torch::zeros({num_rows, H}, dy.options().dtype(at::kFloat));
  }
  const bool pre = sorted_ids.has_value();
  const bool det = ordered || mipipe::g_deterministic || pre;
  TORCH_CHECK(scale == 1.0 || det, "embedding_bwd: scale needs the ordered path");
  // tables of <= 8 rows: per-block partial tables summed in block order, in every mode (cheaper
  // than 256 blocks' atomics onto the same few rows, and deterministic anyway)
  if ((det || num_rows <= 8) && n > 0) {
    auto dyc = dy.contiguous();
    if (num_rows <= 8 && !pre) {
      auto part = torch::empty({mipipe::embedding_bwd_small_blocks(n), num_rows * H},
                               dy.options().dtype(at::kFloat));
      if (scale != 1.0) dyc = (dyc.to(at::kFloat) * scale).to(at::kBFloat16);
      mipipe::embedding_bwd(dyc.data_ptr(), idx.data_ptr<int64_t>(), o.data_ptr<float>(), n,
                            (int)H, (int)num_rows, stream(), part.data_ptr<float>());
    } else {
      Tensor sid, pm;
      if (pre) {
        sid = sorted_ids->contiguous();
        pm = perm->contiguous();
        TORCH_CHECK(sid.numel() == n && pm.numel() == n && sid.scalar_type() == at::kLong &&
                        pm.scalar_type() == at::kLong && sid.is_cuda() && pm.is_cuda(),
                    "embedding_bwd: sorted_ids / perm must be int64 [n] on the GPU");
      } else {
        auto srt = at::sort(idx.reshape({-1}), /*stable=*/true, /*dim=*/0, /*descending=*/false);
        sid = std::get<0>(srt).contiguous();
        pm = std::get<1>(srt).contiguous();
      }
      auto ws = torch::empty({mipipe::embedding_bwd_sorted_ws_floats(n, (int)H)},
                             dy.options().dtype(at::kFloat));
      mipipe::embedding_bwd_sorted(dyc.data_ptr(), sid.data_ptr<int64_t>(), pm.data_ptr<int64_t>(),
                                   o.data_ptr<float>(), ws.data_ptr<float>(), n, (int)H,
                                   (float)scale, stream());
    }
    return o;
  }
  mipipe::embedding_bwd(dy.data_ptr(), idx.data_ptr<int64_t>(), o.data_ptr<float>(), n, (int)H,
                        (int)num_rows, stream());
  return o;
}

// out[c] (+)= Σ_rows x[:, c]; accumulates into ``out`` when given (e.g. a flat-grad view)
Tensor colsum(Tensor x, optional<Tensor> out, bool two_pass) {
  check_cuda(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat, "colsum dtype");
  int64_t cols = x.size(-1), rows = x.numel() / cols;
  TORCH_CHECK(cols % 8 == 0, "colsum needs cols % 8 == 0");
  Tensor o;
  if (out.has_value()) {
    check_vec(*out, cols, "out");
    o = *out;
  } else {
    o = torch::zeros({cols}, x.options().dtype(at::kFloat));
  }
  optional<Tensor> work;
  if (mipipe::g_deterministic || two_pass)
    work = torch::empty({(int64_t)mipipe::colsum_blocks(rows, (int)cols), cols}, x.options().dtype(at::kFloat));
  mipipe::colsum_f32(x.data_ptr(), x.scalar_type() == at::kBFloat16, o.data_ptr<float>(), rows,
                     (int)cols, work.has_value() ? work->data_ptr<float>() : nullptr, stream());
  return o;
}

std::tuple<Tensor, optional<Tensor>> stem_pack(Tensor x, int64_t pad, int64_t Hp, int64_t Wsp,
                                               at::ScalarType dtype, optional<Tensor> w) {
  check_cuda(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.dim() == 4 && x.size(1) <= 4, "stem_pack expects NCHW with C <= 4");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, "x dtype");
  TORCH_CHECK(dtype == at::kBFloat16 || dtype == at::kFloat, "stem_pack produces bf16 / fp32");
  auto y = torch::empty({x.size(0), Hp, Wsp, 8}, x.options().dtype(dtype));
  optional<Tensor> wp;
  long ws[4] = {0, 0, 0, 0};
  if (w.has_value()) {  // the stem filter packed by the same launch
    // (any strides: the parameter is channels_last)
    TORCH_CHECK(w->is_cuda() && w->scalar_type() == at::kFloat && w->device() == x.device(),
                "stem filter: fp32 on x's device");
    TORCH_CHECK(w->dim() == 4 && w->size(1) == x.size(1) && w->size(2) == w->size(3),
                "stem filter must be [Co, C, K, K]");
    for (int d = 0; d < 4; ++d) ws[d] = (long)w->stride(d);
    wp = torch::empty({w->size(0), w->size(2), (w->size(3) + 1) / 2, 8}, x.options().dtype(dtype));
  }
  mipipe::stem_pack(x.data_ptr(), x.scalar_type() == at::kBFloat16, y.data_ptr(), (int)x.size(0),
                    (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)pad, (int)Hp, (int)Wsp,
                    stream(), dtype == at::kFloat, w.has_value() ? w->data_ptr<float>() : nullptr,
                    wp.has_value() ? wp->data_ptr() : nullptr,
                    w.has_value() ? (int)w->size(0) : 0, w.has_value() ? (int)w->size(2) : 0, ws);
  return {y, wp};
}

void stem_wgrad_unpack(Tensor dwp, Tensor g) {
  check_f32(dwp, "dwp");
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat && g.dim() == 4, "g: fp32 [Co,C,K,K]");
  c10::DeviceGuard dg(g.device());
  const int Co = (int)g.size(0), C = (int)g.size(1), K = (int)g.size(2);
  TORCH_CHECK(C <= 4 && g.size(3) == K && dwp.numel() == (int64_t)Co * K * ((K + 1) / 2) * 8,
              "dwp must be the packed [Co, K, ceil(K/2), 8] stem filter gradient");
  long gs[4];
  for (int d = 0; d < 4; ++d) gs[d] = (long)g.stride(d);
  mipipe::stem_wgrad_unpack(dwp.data_ptr<float>(), g.data_ptr<float>(), Co, C, K, gs, stream());
}

void check_attn(const Tensor& qkv, int64_t B, int64_t S, int64_t H) {
  check_bf16(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == B * S && qkv.size(1) == 3 * H * 64,
              "qkv must be [B*S, 3*H*64] (head_dim 64), got ", qkv.sizes());
  TORCH_CHECK(S >= 1 && S <= 2048, "attention supports 1 <= S <= 2048, got ", S);
  TORCH_CHECK(B * S * H * 64 < (1ll << 31), "attention problem too large");
}

const float* mask_ptr(const optional<Tensor>& mask, int64_t B, int64_t S) {
  if (!mask.has_value()) return nullptr;
  check_f32(*mask, "mask");
  TORCH_CHECK(mask->numel() == B * S, "mask must be [B, S]");
  return mask->data_ptr<float>();
}

std::tuple<Tensor, Tensor> attention_fwd(Tensor qkv, int64_t B, int64_t S, int64_t H,
                                         optional<Tensor> mask, double scale, double p_drop,
                                         int64_t seed, optional<Tensor> seed_dev) {
  check_attn(qkv, B, S, H);
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(p_drop >= 0.0 && p_drop < 1.0, "dropout p must be in [0, 1)");
  auto o = torch::empty({B * S, H * 64}, qkv.options());
  auto lse = torch::empty({B, H, S}, qkv.options().dtype(at::kFloat));
  mipipe::attention_fwd(qkv.data_ptr(), mask_ptr(mask, B, S), o.data_ptr(), lse.data_ptr<float>(),
                        (int)B, (int)S, (int)H, (float)scale, (float)p_drop, (uint32_t)seed,
                        stream(), (const uint32_t*)i32_dev(seed_dev, "seed_dev"));
  return {o, lse};
}

Tensor attention_bwd(Tensor dout, Tensor qkv, Tensor o, Tensor lse, int64_t B, int64_t S,
                     int64_t H, optional<Tensor> mask, double scale, double p_drop, int64_t seed,
                     optional<Tensor> seed_dev) {
  check_attn(qkv, B, S, H);
  check_bf16(dout, "dout");
  check_bf16(o, "o");
  check_f32(lse, "lse");
  c10::DeviceGuard g(qkv.device());
  TORCH_CHECK(dout.numel() == B * S * H * 64 && o.numel() == B * S * H * 64, "dout/o shape");
  TORCH_CHECK(lse.numel() == B * H * S, "lse shape");
  auto dqkv = torch::empty_like(qkv);
  auto f = qkv.options().dtype(at::kFloat);
  auto delta = torch::empty({B, H, S}, f);
  auto dq_acc = torch::empty({mipipe::attention_dq_slabs((int)S), B * S, H * 64}, f);
  mipipe::attention_bwd(dout.data_ptr(), qkv.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                        mask_ptr(mask, B, S), dqkv.data_ptr(), delta.data_ptr<float>(),
                        dq_acc.data_ptr<float>(), (int)B, (int)S, (int)H, (float)scale,
                        (float)p_drop, (uint32_t)seed, stream(),
                        (const uint32_t*)i32_dev(seed_dev, "seed_dev"));
  return dqkv;
}

Tensor dropout_fwd(Tensor x, double p, int64_t seed, optional<Tensor> seed_dev) {
  check_bf16(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout p must be in [0, 1)");
  TORCH_CHECK(x.numel() % 8 == 0, "dropout needs numel % 8 == 0");
  auto y = torch::empty_like(x);
  mipipe::dropout_fwd(x.data_ptr(), y.data_ptr(), x.numel(), (float)p, (uint32_t)seed, stream(),
                      (const uint32_t*)i32_dev(seed_dev, "seed_dev"));
  return y;
}

// ------------------------------------------------------------------------------- vision.hip
mipipe::GConvShape gconv_shape(int64_t N, int64_t H, int64_t W, int64_t Ci, int64_t Co, int64_t KH,
                               int64_t KW, int64_t Cig, const std::vector<int64_t>& stride,
                               const std::vector<int64_t>& pad, int64_t groups) {
  TORCH_CHECK(stride.size() == 2 && pad.size() == 2, "stride / pad must be (h, w)");
  TORCH_CHECK(groups >= 1 && Ci % groups == 0 && Co % groups == 0,
              "channels must divide into groups");
  TORCH_CHECK(Cig * groups == Ci, "weight Ci/groups ", Cig, " x ", groups, " != input channels ", Ci);
  mipipe::GConvShape s;
  s.N = (int)N; s.H = (int)H; s.W = (int)W; s.Ci = (int)Ci;
  s.Co = (int)Co; s.KH = (int)KH; s.KW = (int)KW;
  s.sh = (int)stride[0]; s.sw = (int)stride[1]; s.ph = (int)pad[0]; s.pw = (int)pad[1];
  s.groups = (int)groups;
  TORCH_CHECK(s.KH >= 1 && s.KW >= 1 && s.sh >= 1 && s.sw >= 1 && s.ph >= 0 && s.pw >= 0,
              "bad kernel / stride / padding");
  // (checked before dividing: a negative numerator truncates toward zero and gives extent 1)
  TORCH_CHECK(s.H + 2 * s.ph >= s.KH && s.W + 2 * s.pw >= s.KW, "padded input (", s.H + 2 * s.ph,
              " x ", s.W + 2 * s.pw, ") is smaller than the kernel (", s.KH, " x ", s.KW, ")");
  s.Ho =(s.H + 2 * s.ph - s.KH) / s.sh + 1;
  s.Wo = (s.W + 2 * s.pw - s.KW) / s.sw + 1;
  TORCH_CHECK(s.Ho > 0 && s.Wo > 0, "empty conv output");
  return s;
}

// the 8-channel vector depthwise kernels: groups == Ci == Co, C % 8 == 0, C/8 <= 256 threads
bool dw_vec8(const mipipe::GConvShape& s) {
  return s.groups == s.Ci && s.Ci == s.Co && s.Ci % 8 == 0 && s.Ci <= 2048;
}

// depthwise weights [C, KH, KW, 1] -> taps-major [KH*KW, C] (one 16-byte vector per tap)
Tensor dw_taps_major(const Tensor& w) {
  return w.reshape({w.size(0), w.size(1) * w.size(2)}).t().contiguous();
}

const void* act_mask_src(const optional<Tensor>& z, int64_t act, const Tensor& like) {
  if (act == 0 || !z.has_value()) return nullptr;
  check_act(*z, "z");
  check_same(*z, like, "z");
  TORCH_CHECK(z->sizes() == like.sizes(), "z must match the conv output");
  return z->data_ptr();
}

Tensor gconv_fwd(Tensor x, Tensor w, std::vector<int64_t> stride, std::vector<int64_t> pad,
                 int64_t groups, optional<Tensor> bias, int64_t act) {
  check_act(x, "x");
  check_same(w, x, "w");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4, "gconv expects NHWC x and [Co,KH,KW,Ci/groups] w");
  auto s = gconv_shape(x.size(0), x.size(1), x.size(2), x.size(3), w.size(0), w.size(1),
                       w.size(2), w.size(3), stride, pad, groups);
  if (bias.has_value()) check_vec(*bias, s.Co, "bias");
  TORCH_CHECK(act >= 0 && act <= 2, "act must be 0 (none), 1 (relu) or 2 (relu6)");
  auto y = torch::empty({s.N, s.Ho, s.Wo, s.Co}, x.options());
  const float* bp = bias.has_value() ? bias->data_ptr<float>() : nullptr;
  if (dw_vec8(s)) {
    auto wt = dw_taps_major(w);
    mipipe::dwconv_fwd(x.data_ptr(), wt.data_ptr(), bp, y.data_ptr(), s, (int)act,
                       stream(), is_f32(x));
  } else {
    mipipe::gconv_fwd(x.data_ptr(), w.data_ptr(), bp, y.data_ptr(), s, (int)act,
                      stream(), is_f32(x));
  }
  return y;
}

Tensor gconv_dgrad(Tensor dy, Tensor w, std::vector<int64_t> x_shape, std::vector<int64_t> stride,
                   std::vector<int64_t> pad, int64_t groups, optional<Tensor> z, int64_t act) {
  check_act(dy, "dy");
  check_same(w, dy, "w");
  c10::DeviceGuard g(dy.device());
  TORCH_CHECK(x_shape.size() == 4 && w.dim() == 4, "x_shape must be [N,H,W,Ci]");
  auto s = gconv_shape(x_shape[0], x_shape[1], x_shape[2], x_shape[3], w.size(0), w.size(1),
                       w.size(2), w.size(3), stride, pad, groups);
  TORCH_CHECK(dy.dim() == 4 && dy.size(0) == s.N && dy.size(1) == s.Ho && dy.size(2) == s.Wo &&
                  dy.size(3) == s.Co, "dy shape does not match the convolution");
  TORCH_CHECK(act >= 0 && act <= 2, "bad act");
  const void* zp = act_mask_src(z, act, dy);
  auto dx = torch::empty({s.N, s.H, s.W, s.Ci}, dy.options());
  if (dw_vec8(s)) {
    auto wt = dw_taps_major(w);
    mipipe::dwconv_dgrad(dy.data_ptr(), wt.data_ptr(), zp, dx.data_ptr(), s, (int)act,
                         stream(), is_f32(dy));
  } else {
    mipipe::gconv_dgrad(dy.data_ptr(), w.data_ptr(), zp, dx.data_ptr(), s, (int)act,
                        stream(), is_f32(dy));
  }
  return dx;
}

std::tuple<Tensor, optional<Tensor>> gconv_wgrad(Tensor dy, Tensor x, int64_t kh, int64_t kw,
                                                 std::vector<int64_t> stride,
                                                 std::vector<int64_t> pad, int64_t groups,
                                                 optional<Tensor> z, int64_t act,
                                                 optional<Tensor> out, optional<Tensor> dbias,
                                                 bool want_bias) {
  check_act(dy, "dy");
  check_same(x, dy, "x");
  c10::DeviceGuard g(dy.device());
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4, "NHWC tensors expected");
  const int64_t Co = dy.size(3), Ci = x.size(3);
  TORCH_CHECK(groups >= 1 && Ci % groups == 0, "bad groups");
  auto s = gconv_shape(x.size(0), x.size(1), x.size(2), Ci, Co, kh, kw, Ci / groups, stride, pad,
                       groups);
  TORCH_CHECK(dy.size(0) == s.N && dy.size(1) == s.Ho && dy.size(2) == s.Wo, "dy/x mismatch");
  TORCH_CHECK(act >= 0 && act <= 2, "bad act");
  const void* zp = act_mask_src(z, act, dy);
  Tensor dw;
  if (out.has_value()) {  // accumulate into the parameter's flat-gradient view
    check_f32(*out, "out");
    TORCH_CHECK(out->dim() == 4 && out->size(0) == Co && out->size(1) == kh &&
                    out->size(2) == kw && out->size(3) == Ci / groups,
                "wgrad out must be [Co,KH,KW,Ci/groups]");
    dw = *out;
  } else {
    dw = torch::zeros({Co, kh, kw, Ci / groups}, x.options().dtype(at::kFloat));
  }
  optional<Tensor> db;
  if (dbias.has_value()) {
    check_vec(*dbias, Co, "dbias");
    db = *dbias;
  } else if (want_bias) {
    db = torch::zeros({Co}, x.options().dtype(at::kFloat));
  }
  float* dbp = db.has_value() ? db->data_ptr<float>() : nullptr;
  if (dw_vec8(s))
    mipipe::dwconv_wgrad(dy.data_ptr(), x.data_ptr(), zp, dw.data_ptr<float>(), dbp, s, (int)act,
                         stream(), is_f32(dy));
  else
    mipipe::gconv_wgrad(dy.data_ptr(), x.data_ptr(), zp, dw.data_ptr<float>(), dbp, s, (int)act,
                        stream(), is_f32(dy));
  return {dw, db};
}

// shifted per-channel sums (one zeroed [2, C] allocation; rows returned as [1, C] views)
std::tuple<Tensor, Tensor> chan_stats(Tensor y, Tensor shift) {
  check_act(y, "y");
  c10::DeviceGuard g(y.device());
  int64_t C = y.size(-1), M = y.numel() / C;
  check_vec(shift, C, "shift");
  // [2][R][C] replica-row partials: bn_finalize sums the R rows
  auto st = torch::zeros({2, (int64_t)mipipe::kStatReplicas, C}, y.options().dtype(at::kFloat));
  auto ps = st[0], pq = st[1];
  // (the generic-C fallback kernel accumulates row 0 only; the other rows stay zero)
  mipipe::chan_stats(y.data_ptr(), shift.data_ptr<float>(), M, (int)C, ps.data_ptr<float>(),
                     pq.data_ptr<float>(), stream(), is_f32(y));
  return {ps, pq};
}

Tensor affine_act(Tensor y, Tensor scale, Tensor bias, int64_t act) {
  check_act(y, "y");
  c10::DeviceGuard g(y.device());
  int64_t C = y.size(-1), M = y.numel() / C;
  check_vec(scale, C, "scale");
  check_vec(bias, C, "bias");
  TORCH_CHECK(act >= 0 && act <= 2, "bad act");
  auto z = torch::empty_like(y);
  mipipe::affine_act(y.data_ptr(), scale.data_ptr<float>(), bias.data_ptr<float>(), z.data_ptr(),
                     M, (int)C, (int)act, stream(), is_f32(y));
  return z;
}

std::tuple<Tensor, Tensor> bn_generic_bwd_reduce(Tensor dz, optional<Tensor> z, Tensor y,
                                                 Tensor mean, Tensor invstd, int64_t act) {
  check_act(y, "y");
  check_same(dz, y, "dz");
  c10::DeviceGuard g(y.device());
  int64_t C = y.size(-1), M = y.numel() / C;
  TORCH_CHECK(dz.sizes() == y.sizes(), "dz / y shape mismatch");
  check_vec(mean, C, "mean");
  check_vec(invstd, C, "invstd");
  TORCH_CHECK(act >= 0 && act <= 2 && (act == 0 || z.has_value()), "activation backward needs z");
  const void* zp = act_mask_src(z, act, y);
  const int R = mipipe::kStatReplicas;  // replica rows for the atomics, summed below
  auto rep = torch::zeros({2, (int64_t)R, C}, y.options().dtype(at::kFloat));
  mipipe::bn_generic_bwd_reduce(dz.data_ptr(), zp, y.data_ptr(), mean.data_ptr<float>(),
                                invstd.data_ptr<float>(), M, (int)C, (int)act,
                                rep[0].data_ptr<float>(), rep[1].data_ptr<float>(), stream(),
                                is_f32(y));
  auto st = torch::empty({2, C}, y.options().dtype(at::kFloat));
  auto sg = st[0], sgx = st[1];
  mipipe::det_sum_rows(rep[0].data_ptr<float>(), rep[1].data_ptr<float>(), R, (int)C,
                       sg.data_ptr<float>(), sgx.data_ptr<float>(), false, stream());
  return {sg, sgx};
}

Tensor bn_generic_bwd_apply(Tensor dz, optional<Tensor> z, Tensor y, Tensor mean, Tensor invstd,
                            Tensor gamma, optional<Tensor> sum_g, optional<Tensor> sum_gx,
                            int64_t count, int64_t act) {
  check_act(y, "y");
  check_same(dz, y, "dz");
  c10::DeviceGuard g(y.device());
  int64_t C = y.size(-1), M = y.numel() / C;
  TORCH_CHECK(dz.sizes() == y.sizes(), "dz / y shape mismatch");
  for (auto* t : {&mean, &invstd, &gamma}) check_vec(*t, C, "bn vector");
  TORCH_CHECK(sum_g.has_value() == sum_gx.has_value(), "pass both sums or none");
  if (sum_g.has_value()) {
    check_vec(*sum_g, C, "sum_g");
    check_vec(*sum_gx, C, "sum_gx");
  }
  TORCH_CHECK(act >= 0 && act <= 2 && (act == 0 || z.has_value()), "activation backward needs z");
  TORCH_CHECK(count > 0, "count must be positive");
  const void* zp = act_mask_src(z, act, y);
  auto dy = torch::empty_like(y);
  mipipe::bn_generic_bwd_apply(dz.data_ptr(), zp, y.data_ptr(), mean.data_ptr<float>(),
                               invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                               sum_g.has_value() ? sum_g->data_ptr<float>() : nullptr,
                               sum_gx.has_value() ? sum_gx->data_ptr<float>() : nullptr, count, M,
                               (int)C, (int)act, dy.data_ptr(), stream(), is_f32(y));
  return dy;
}

Tensor avgpool2d_fwd(Tensor x, int64_t k, int64_t s, int64_t p) {
  check_act(x, "x");
  c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.dim() == 4, "x must be NHWC");
  TORCH_CHECK(k >= 1 && s >= 1 && p >= 0 && 2 * p <= k, "bad avgpool geometry");
  int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
  int Ho = pool_out(H, k, s, p, false), Wo = pool_out(W, k, s, p, false);
  TORCH_CHECK(Ho > 0 && Wo > 0, "empty avgpool output");
  auto y = torch::empty({N, Ho, Wo, C}, x.options());
  mipipe::avgpool2d_fwd(x.data_ptr(), y.data_ptr(), N, H, W, C, Ho, Wo, (int)k, (int)s, (int)p,
                        stream(), is_f32(x));
  return y;
}

Tensor avgpool2d_bwd(Tensor dy, std::vector<int64_t> xs, int64_t k, int64_t s, int64_t p) {
  check_act(dy, "dy");
  c10::DeviceGuard g(dy.device());
  TORCH_CHECK(xs.size() == 4 && dy.dim() == 4, "NHWC shapes expected");
  TORCH_CHECK(k >= 1 && s >= 1 && p >= 0 && 2 * p <= k, "bad avgpool geometry");
  int N = xs[0], H = xs[1], W = xs[2], C = xs[3];
  int Ho = pool_out(H, k, s, p, false), Wo = pool_out(W, k, s, p, false);
  TORCH_CHECK(dy.size(0) == N && dy.size(1) == Ho && dy.size(2) == Wo && dy.size(3) == C,
              "avgpool2d_bwd shape mismatch");
  auto dx = torch::empty({N, H, W, C}, dy.options());
  mipipe::avgpool2d_bwd(dy.data_ptr(), dx.data_ptr(), N, H, W, C, Ho, Wo, (int)k, (int)s, (int)p,
                        stream(), is_f32(dy));
  return dx;
}

}  // namespace

namespace mipipe_bind {
void bind_loss(py::module& m);  // csrc/bind/loss.cpp: cross-entropy, top-1, evaluation statistics
void bind_data(py::module& m);  // csrc/bind/data.cpp: layout, synthetic data, records, batch mix
void bind_vit(py::module& m);   // csrc/bind/vit.cpp: patchify, token assembly
void bind_convnext(py::module& m);  // csrc/bind/convnext.cpp: dwconv7, scale_residual
void bind_se(py::module& m);    // csrc/bind/se.cpp: bn_act_pool, se_scale
}

namespace mipipe_comm {
void init_comm(py::module& m);  // csrc/comm/reducer.cpp: native DDP reducer, bf16 wire passes
void init_oneshot(py::module& m);  // csrc/comm/oneshot.cpp: one-shot IPC collectives
}

PYBIND11_MODULE(_C, m) {
  m.doc() = "mipipe gfx950 (MI355X) HIP kernels";
  mipipe_comm::init_comm(m);
  mipipe_comm::init_oneshot(m);
  mipipe_bind::bind_loss(m);
  mipipe_bind::bind_data(m);
  mipipe_bind::bind_vit(m);
  mipipe_bind::bind_convnext(m);
  mipipe_bind::bind_se(m);
  m.def("conv_fwd", &conv_fwd, py::arg("x"), py::arg("w"), py::arg("stride"), py::arg("pad"),
        py::arg("shift") = py::none(), py::arg("slab_sum") = py::none(),
        py::arg("slab_sq") = py::none(), py::arg("bias") = py::none(), py::arg("relu") = false,
        py::arg("stride_w") = 0, py::arg("pad_w") = -1, py::arg("cfg") = -1,
        py::arg("wflip") = py::none(), py::arg("in_scale") = py::none(),
        py::arg("in_bias") = py::none());
  m.def("conv_fwd_infer", &conv_fwd_infer, py::arg("x"), py::arg("w"), py::arg("stride"),
        py::arg("pad"), py::arg("scale") = py::none(), py::arg("shift") = py::none(),
        py::arg("residual") = py::none(), py::arg("relu") = false, py::arg("stride_w") = 0,
        py::arg("pad_w") = -1, py::arg("cfg") = -1);
  m.attr("STAT_REPLICAS") = mipipe::kStatReplicas;
  // launch constants of vision.hip / pool.hip (launchers.hpp): the edge tests derive shapes from them
  m.attr("V8_ROW_U") = mipipe::kV8RowU;
  m.attr("V8_APPLY_U") = mipipe::kV8ApplyU;
  m.attr("V8_REDUCE_BLOCKS") = mipipe::kV8ReduceBlocks;
  m.attr("V8_APPLY_BLOCKS") = mipipe::kV8ApplyBlocks;
  m.attr("CHAN_GRID_BLOCKS") = mipipe::kChanGridBlocks;
  m.attr("GRID_FOR_BLOCKS") = mipipe::kGridForBlocks;
  m.attr("EW_GRID_BLOCKS") = mipipe::kEwGridBlocks;
  // launch constants of bn.hip, and the grid / unroll actually in effect
  m.attr("BN_THREADS") = mipipe::kBnThreads;
  m.attr("BN_ROW_U") = mipipe::kBnRowU;
  m.attr("BN_APPLY_U") = mipipe::kBnApplyU;
  m.attr("BN_REDUCE_BLOCKS") = mipipe::kBnReduceBlocks;
  m.attr("BN_ATOMIC_BUDGET") = (int64_t)mipipe::kBnAtomicBudget;
  m.attr("BN_MIN_BLOCKS") = mipipe::kBnMinBlocks;
  m.attr("BN_ROW_ITERS") = mipipe::kBnRowIters;
  m.attr("DET_CHUNK_ROWS") = mipipe::kDetChunkRows;
  m.def("bn_bwd_reduce_blocks", [](int64_t M, int64_t C) {
    TORCH_CHECK(M >= 0 && C >= 8 && C % 8 == 0, "bn_bwd_reduce_blocks: M >= 0, C % 8 == 0");
    return mipipe::bn_bwd_reduce_blocks((long)M, (int)C);
  });
  m.def("bn_apply_u", []() { return mipipe::bn_apply_u(); });
  m.def("conv_dgrad", &conv_dgrad, py::arg("dy"), py::arg("w"), py::arg("x_shape"),
        py::arg("stride"), py::arg("pad"), py::arg("addend") = py::none(),
        py::arg("bn_y") = py::none(), py::arg("bn_mean") = py::none(),
        py::arg("bn_invstd") = py::none(), py::arg("bn_scale") = py::none(),
        py::arg("bn_bias") = py::none(), py::arg("bn_rep") = py::none(),
        py::arg("bn_z") = py::none(), py::arg("pad_w") = -1, py::arg("cfg") = -1,
        py::arg("bn_mask") = py::none(), py::arg("bn_y2") = py::none(),
        py::arg("bn_mean2") = py::none(), py::arg("bn_invstd2") = py::none(),
        py::arg("wflip_pre") = py::none());
  m.def("dgrad_preflip_ok", [](std::vector<int64_t> x_shape, std::vector<int64_t> w_shape,
                               int stride, int pad) {
    // whether conv_fwd(wflip=...) prepares this conv's data-grad weight (dgrad_preflip_ok)
    return mipipe::dgrad_preflip_ok(make_conv_shape(x_shape[0], x_shape[1], x_shape[2], x_shape[3],
                                                    w_shape[0], (int)w_shape[1], (int)w_shape[2],
                                                    stride, pad, 0, -1, false));
  });
  m.def("bn_bwd_collect", &bn_bwd_collect, py::arg("rep"), py::arg("C"),
        py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none());
  m.def("conv_wgrad", &conv_wgrad, py::arg("dy"), py::arg("x"), py::arg("kh"), py::arg("kw"),
        py::arg("stride"), py::arg("pad"), py::arg("out") = py::none(), py::arg("stride_w") = 0,
        py::arg("pad_w") = -1, py::arg("cfg") = -1, py::arg("col_rep") = py::none(),
        py::arg("col_out") = py::none(), py::arg("col_dgamma") = py::none(),
        py::arg("col_dbeta") = py::none(), py::arg("col_two") = false,
        py::arg("col_dgamma2") = py::none(), py::arg("col_dbeta2") = py::none(),
        py::arg("in_scale") = py::none(), py::arg("in_bias") = py::none());
  m.attr("CONV_TILE_CONFIGS") = mipipe::kConvTileConfigs;
  m.def("set_benchmark", [](bool on, bool verbose, int reps) {
    tune::g_benchmark = on;
    tune::g_verbose = verbose;
    tune::g_reps = std::max(1, reps);
  }, py::arg("on"), py::arg("verbose") = false, py::arg("reps") = 3);
  m.def("get_benchmark", []() { return tune::g_benchmark; });
  m.def("set_force_tune", [](bool on) { tune::g_force_tune = on; });
  m.def("set_wgrad3x3", [](bool on) { mipipe::g_wgrad3x3 = on; });
  m.def("get_wgrad3x3", []() { return mipipe::g_wgrad3x3; });
  m.def("set_nt_store", [](int mask) { mipipe::g_nt_store = mask; });
  m.def("set_nt_min_bytes", [](long b) { mipipe::g_nt_min_bytes = b; });
  m.def("get_nt_min_bytes", []() { return mipipe::g_nt_min_bytes; });
  m.def("get_nt_store", []() { return mipipe::g_nt_store; });
  m.def("set_ws_finish", [](bool on) { g_ws_finish = on; });
  m.def("get_ws_finish", []() { return g_ws_finish; });
  m.def("set_layernorm_mode", [](int64_t m) { mipipe::set_layernorm_mode((int)m); });
  m.def("get_layernorm_mode", []() { return mipipe::get_layernorm_mode(); });
  m.def("set_deterministic", [](bool on) { mipipe::g_deterministic = on ? 1 : 0; });
  m.def("get_deterministic", []() { return mipipe::g_deterministic != 0; });
  m.def("tune_table", []() { return tune::g_table; });
  m.def("set_tune_entry", [](const std::string& k, int cfg) {
    TORCH_CHECK(mipipe::plan_id_ok(cfg, mipipe::kConvTileConfigs), "bad tile plan id");
    if (cfg < 0) tune::g_table.erase(k);
    else tune::g_table[k] = cfg;
  });
  m.def("clear_tune_table", []() { tune::g_table.clear(); });
  m.def("bn_finalize", &bn_finalize, py::arg("psum"), py::arg("psq"), py::arg("count"),
        py::arg("shift"), py::arg("gamma"), py::arg("beta"), py::arg("rm"), py::arg("rv"),
        py::arg("momentum"), py::arg("eps"), py::arg("zero_after") = true,
        py::arg("nbt") = py::none());
  m.def("bn_fold_affine", &bn_fold_affine, py::arg("weight"), py::arg("bias"),
        py::arg("running_mean"), py::arg("running_var"), py::arg("eps"),
        py::arg("conv_bias") = py::none());
  m.def("bn_act_fwd", &bn_act_fwd, py::arg("y"), py::arg("scale"), py::arg("bias"),
        py::arg("relu"), py::arg("r"), py::arg("rscale"), py::arg("rbias"),
        py::arg("mask") = py::none());
  m.def("bn_act_bwd_reduce", &bn_act_bwd_reduce, py::arg("dz"), py::arg("z"), py::arg("y"),
        py::arg("mean"), py::arg("invstd"), py::arg("relu"), py::arg("y2") = py::none(),
        py::arg("mean2") = py::none(), py::arg("invstd2") = py::none(),
        py::arg("rep") = py::none(), py::arg("dgamma") = py::none(), py::arg("dbeta") = py::none(),
        py::arg("dgamma2") = py::none(), py::arg("dbeta2") = py::none());
  m.def("bn_act_bwd_apply", &bn_act_bwd_apply);
  m.def("maxpool_fwd", &maxpool_fwd, py::arg("x"), py::arg("k"), py::arg("s"), py::arg("p"),
        py::arg("ceil_mode") = false);
  m.def("gconv_fwd", &gconv_fwd, py::arg("x"), py::arg("w"), py::arg("stride"), py::arg("pad"),
        py::arg("groups"), py::arg("bias") = py::none(), py::arg("act") = 0);
  m.def("gconv_dgrad", &gconv_dgrad, py::arg("dy"), py::arg("w"), py::arg("x_shape"),
        py::arg("stride"), py::arg("pad"), py::arg("groups"), py::arg("z") = py::none(),
        py::arg("act") = 0);
  m.def("gconv_wgrad", &gconv_wgrad, py::arg("dy"), py::arg("x"), py::arg("kh"), py::arg("kw"),
        py::arg("stride"), py::arg("pad"), py::arg("groups"), py::arg("z") = py::none(),
        py::arg("act") = 0, py::arg("out") = py::none(), py::arg("dbias") = py::none(),
        py::arg("want_bias") = false);
  m.def("chan_stats", &chan_stats);
  m.def("affine_act", &affine_act);
  m.def("bn_generic_bwd_reduce", &bn_generic_bwd_reduce);
  m.def("bn_generic_bwd_apply", &bn_generic_bwd_apply);
  m.def("avgpool2d_fwd", &avgpool2d_fwd);
  m.def("avgpool2d_bwd", &avgpool2d_bwd);
  m.def("maxpool_bwd_impl", &maxpool_bwd);
  m.def("pool_bn_fwd", &pool_bn_fwd, py::arg("y"), py::arg("scale"), py::arg("bias"), py::arg("k"),
        py::arg("s"), py::arg("p"));
  m.def("pool_bn_bwd", &pool_bn_bwd, py::arg("dp"), py::arg("idx"), py::arg("pout"), py::arg("y"),
        py::arg("mean"), py::arg("invstd"), py::arg("gamma"), py::arg("rep"), py::arg("count"),
        py::arg("k"), py::arg("s"), py::arg("p"), py::arg("dgamma") = py::none(),
        py::arg("dbeta") = py::none());
  m.def("stem_fused_supported", &stem_fused_supported);
  m.def("stem_fwd_stats", &stem_fwd_stats);
  m.def("stem_fwd_pool", &stem_fwd_pool, py::arg("xp"), py::arg("w"), py::arg("scale"),
        py::arg("bias"), py::arg("want_y") = true);
  m.def("stem_bwd", &stem_bwd, py::arg("xp"), py::arg("y"), py::arg("dp"), py::arg("idx"),
        py::arg("pout"), py::arg("mean"), py::arg("invstd"), py::arg("gamma"), py::arg("beta"),
        py::arg("rep"), py::arg("count"), py::arg("dgamma") = py::none(),
        py::arg("dbeta") = py::none());
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);
  m.def("gemm", &gemm, py::arg("a"), py::arg("b"), py::arg("trans_a"), py::arg("trans_b"),
        py::arg("bias"), py::arg("act"), py::arg("out_dtype"), py::arg("c"), py::arg("beta"),
        py::arg("plan") = -1, py::arg("addend") = py::none(),
        py::arg("prefetch") = py::none());
  m.def("touch", &touch, py::arg("tensors"));
  m.def("sgd_step", &sgd_step);
  m.def("adamw_step", &adamw_step, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
        py::arg("shadow"), py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
        py::arg("wd"), py::arg("step"), py::arg("grad_scale"), py::arg("step_dev") = py::none());
  m.def("lars_step", &lars_step, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("shadow"),
        py::arg("chunks"), py::arg("segs"), py::arg("part"), py::arg("segtot"), py::arg("ratio"),
        py::arg("scal"), py::arg("step_dev"), py::arg("momentum"), py::arg("tc"), py::arg("eps"),
        py::arg("max_norm"), py::arg("grad_scale"), py::arg("kind"), py::arg("base_lr"),
        py::arg("end_lr"), py::arg("warmup"), py::arg("total"));
  m.def("lamb_step", &lamb_step, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"),
        py::arg("shadow"), py::arg("chunks"), py::arg("segs"), py::arg("part"),
        py::arg("segtot"), py::arg("ratio"), py::arg("scal"), py::arg("step_dev"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("max_norm"), py::arg("grad_scale"),
        py::arg("kind"), py::arg("base_lr"), py::arg("end_lr"), py::arg("warmup"),
        py::arg("total"));
  m.attr("OPTIM_CHUNK") = mipipe::kOptimChunk;
  m.def("ema_update", &ema_update, py::arg("p"), py::arg("ema"), py::arg("calls_dev"),
        py::arg("every"), py::arg("w_min"), py::arg("warmup"), py::arg("scal"));
  m.def("ema_swap", &ema_swap, py::arg("p"), py::arg("ema"), py::arg("shadow"));
  m.def("ema_buffers_update", &ema_buffers_update, py::arg("table"), py::arg("ema_buffers"),
        py::arg("calls_dev"), py::arg("every"), py::arg("w_min"), py::arg("warmup"));
  m.def("ema_buffers_swap", &ema_buffers_swap, py::arg("table"), py::arg("ema_buffers"));
  m.attr("EMA_ROW_MAX") = mipipe::kEmaRowMax;
  m.def("gelu_fwd", &gelu_fwd);
  m.def("gelu_bwd", &gelu_bwd);
  m.def("gemm_gelu", &gemm_gelu, py::arg("a"), py::arg("b"), py::arg("bias") = py::none(),
        py::arg("plan") = -1);
  m.def("gelu_bwd_colsum", &gelu_bwd_colsum, py::arg("dy"), py::arg("x"), py::arg("bias"));
  m.def("layernorm_fwd", &layernorm_fwd, py::arg("x"), py::arg("gamma"), py::arg("beta"),
        py::arg("eps"), py::arg("res") = py::none(), py::arg("drop_p") = 0.0,
        py::arg("drop_seed") = 0, py::arg("drop_seed_dev") = py::none());
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dy"), py::arg("x"), py::arg("mean"),
        py::arg("rstd"), py::arg("gamma"), py::arg("dgamma") = py::none(),
        py::arg("dbeta") = py::none(), py::arg("drop_p") = 0.0, py::arg("drop_seed") = 0,
        py::arg("drop_seed_dev") = py::none(), py::arg("dbias") = py::none(),
        py::arg("dsum") = py::none());
  m.def("embedding_bwd", &embedding_bwd, py::arg("dy"), py::arg("idx"), py::arg("num_rows"),
        py::arg("out") = py::none(), py::arg("ordered") = false, py::arg("scale") = 1.0,
        py::arg("sorted_ids") = py::none(), py::arg("perm") = py::none());
  m.def("colsum", &colsum, py::arg("x"), py::arg("out") = py::none(),
        py::arg("two_pass") = false);
  m.def("set_colsum_row_blocks", [](int v) { mipipe::g_colsum_row_blocks = v; });
  m.def("set_attn_waves", [](int v) { mipipe::g_attn_waves = v; });
  m.def("attention_fwd", &attention_fwd, py::arg("qkv"), py::arg("B"), py::arg("S"), py::arg("H"),
        py::arg("mask") = py::none(), py::arg("scale") = 0.125, py::arg("p_drop") = 0.0,
        py::arg("seed") = 0, py::arg("seed_dev") = py::none());
  m.def("attention_bwd", &attention_bwd, py::arg("dout"), py::arg("qkv"), py::arg("o"),
        py::arg("lse"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("mask") = py::none(),
        py::arg("scale") = 0.125, py::arg("p_drop") = 0.0, py::arg("seed") = 0,
        py::arg("seed_dev") = py::none());
  m.def("dropout_fwd", &dropout_fwd, py::arg("x"), py::arg("p"), py::arg("seed"),
        py::arg("seed_dev") = py::none());
  m.def("stem_pack", &stem_pack, py::arg("x"), py::arg("pad"), py::arg("Hp"), py::arg("Wsp"),
        py::arg("dtype") = at::kBFloat16, py::arg("w") = py::none());
  m.def("stem_wgrad_unpack", &stem_wgrad_unpack, py::arg("dwp"), py::arg("g"));
  m.def("set_splitk_target", [](int v) { mipipe::g_splitk_target = std::max(1, v); });
  m.def("get_splitk_target", []() { return mipipe::g_splitk_target; });
  m.def("set_wgrad_xcd", [](bool on) { mipipe::g_wgrad_xcd = on ? 1 : 0; });
  m.def("get_wgrad_xcd", []() { return mipipe::g_wgrad_xcd != 0; });
  m.def("set_stat_rows", [](int v) {
    TORCH_CHECK(v >= 1 && v <= mipipe::kStatReplicas, "stat rows must be in [1, ", mipipe::kStatReplicas, "]");
    mipipe::g_stat_rows = v;
  });
  m.def("set_ns1_max_k", [](int v) { mipipe::g_ns1_max_k = v; });
  m.def("set_ns1_max_k_gather", [](int v) { mipipe::g_ns1_max_k_gather = v; });
}
