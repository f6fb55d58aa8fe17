// Native multi-threaded record loader: the C++ counterpart of task.py's DataLoader(num_workers=8)
// + torchvision transforms (task.py:246-267: RandomCrop(32, padding=4), RandomHorizontalFlip,
// ToTensor, Normalize(mean, std), DistributedSampler shards).
//
// Input: fixed-size binary records, CIFAR-10 binary layout ([label bytes][C planes of H*W
// uint8]); the files are memory-mapped, never read whole.  A pool of worker threads decodes
// whole batches (crop / flip / normalise to float32 NCHW, int64 labels) into a ring of
// `prefetch` batch slots, in order; the consumer copies the next batch into caller memory
// (a pinned host tensor, then one async H2D copy) with the GIL released.
// Augmentation randomness is a pure function of (seed, epoch, sample index), so a resumed or
// re-sharded run sees the same crops/flips for the same sample and epoch.
// Raw mode (LoaderConfig::raw): the workers only gather — whole records and their global sample
// indices go through the same ring, and the transform runs on the GPU (csrc/kernels/records.hip).
// LoaderConfig::transform "rrc": RandomResizedCrop + flip + Normalize to out_h x out_w instead of
// the same-size crop (fill_rrc; geometry in csrc/common/rrc.hpp, shared with the device kernel).
// LoaderConfig::auto_augment / erase_pq (training, non-raw modes): TrivialAugmentWide on the stored
// image before the transform and Random Erasing on its output, from csrc/common/augment.hpp — the
// functions the device kernels (csrc/kernels/augment.hip) use, so both decode modes agree.
#include "runtime.hpp"

#include "../common/augment.hpp"
#include "../common/rrc.hpp"

#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <stdexcept>

namespace mipipe_rt {

static inline uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

RecordLoader::RecordLoader(const LoaderConfig& cfg) : cfg_(cfg) {
  if (cfg_.C <= 0 || cfg_.H <= 0 || cfg_.W <= 0 || cfg_.batch <= 0)
    throw std::invalid_argument("bad loader geometry");
  if ((int)cfg_.mean.size() != cfg_.C || (int)cfg_.stdv.size() != cfg_.C)
    throw std::invalid_argument("mean/std must have C entries");
  if (cfg_.transform != "crop" && cfg_.transform != "rrc")
    throw std::invalid_argument("transform must be \"crop\" or \"rrc\"");
  rrc_ = cfg_.transform == "rrc";
  if (rrc_) {
    if (cfg_.out_h == 0) cfg_.out_h = cfg_.H;
    if (cfg_.out_w == 0) cfg_.out_w = cfg_.W;
    const int lim = 32768;  // rrc.hpp's products stay inside 64 bits
    if (std::min(cfg_.H, cfg_.W) < 2 || cfg_.out_h < 1 || cfg_.out_w < 1 ||
        std::max(std::max(cfg_.H, cfg_.W), std::max(cfg_.out_h, cfg_.out_w)) > lim)
      throw std::invalid_argument("rrc needs stored extents in [2, 32768] and output extents in [1, 32768]");
  } else if ((cfg_.out_h && cfg_.out_h != cfg_.H) || (cfg_.out_w && cfg_.out_w != cfg_.W)) {
    throw std::invalid_argument("out_h / out_w need transform \"rrc\"");
  }
  if (!cfg_.auto_augment.empty() && cfg_.auto_augment != "ta_wide")
    throw std::invalid_argument("auto_augment must be \"\" or \"ta_wide\"");
  augment_ = cfg_.train && !cfg_.auto_augment.empty();
  if (augment_ && cfg_.C != 1 && cfg_.C != 3)
    throw std::invalid_argument("auto_augment needs 1 or 3 channels");
  if (cfg_.erase_pq > (1u << 24)) throw std::invalid_argument("erase_pq must be in [0, 2^24]");
  if (!cfg_.train) cfg_.erase_pq = 0;
  if (cfg_.erase_pq && std::max(rrc_ ? cfg_.out_h : cfg_.H, rrc_ ? cfg_.out_w : cfg_.W) > 32768)
    throw std::invalid_argument("erase_pq needs output extents <= 32768");
  out_per_ = rrc_ ? (size_t)cfg_.C * cfg_.out_h * cfg_.out_w : (size_t)cfg_.C * cfg_.H * cfg_.W;
  rec_bytes_ = (size_t)cfg_.label_bytes + (size_t)cfg_.C * cfg_.H * cfg_.W;
  for (auto& f : cfg_.files) {
    int fd = open(f.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd < 0) throw std::runtime_error("cannot open " + f);
    struct stat st;
    fstat(fd, &st);
    size_t sz = (size_t)st.st_size;
    if (sz < (size_t)cfg_.header_bytes || (sz - cfg_.header_bytes) % rec_bytes_ != 0) {
      close(fd);
      throw std::runtime_error(f + ": size is not header + k * record_bytes");
    }
    void* p = sz ? mmap(nullptr, sz, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
    close(fd);
    if (sz && p == MAP_FAILED) throw std::runtime_error("mmap failed for " + f);
    if (sz) madvise(p, sz, MADV_WILLNEED);
    maps_.push_back({(const uint8_t*)p, sz});
    int64_t n = (int64_t)((sz - cfg_.header_bytes) / rec_bytes_);
    file_start_.push_back(total_);
    total_ += n;
  }
  slot_x_.resize(cfg_.prefetch);
  slot_y_.resize(cfg_.prefetch);
  slot_raw_.resize(cfg_.prefetch);
  slot_n_.assign(cfg_.prefetch, 0);
  slot_batch_.assign(cfg_.prefetch, -1);
  for (int s = 0; s < cfg_.prefetch; ++s) {
    if (cfg_.raw) slot_raw_[s].resize((size_t)cfg_.batch * rec_bytes_);  // no float slots
    else slot_x_[s].resize((size_t)cfg_.batch * out_per_);
    slot_y_[s].resize(cfg_.batch);
  }
  for (int w = 0; w < std::max(1, cfg_.workers); ++w) threads_.emplace_back([this] { worker(); });
}

RecordLoader::~RecordLoader() {
  {
    std::lock_guard<std::mutex> g(mu_);
    shutdown_ = true;
  }
  cv_work_.notify_all();
  cv_slot_.notify_all();
  for (auto& t : threads_) t.join();
  for (auto& m : maps_)
    if (m.first) munmap((void*)m.first, m.second);
}

const uint8_t* RecordLoader::record(int64_t i) const {
  if (i < 0 || i >= total_) throw std::out_of_range("record index");
  size_t f = std::upper_bound(file_start_.begin(), file_start_.end(), i) - file_start_.begin() - 1;
  return maps_[f].first + cfg_.header_bytes + (size_t)(i - file_start_[f]) * rec_bytes_;
}

void RecordLoader::start_epoch(const std::vector<int64_t>& indices, int64_t epoch) {
  for (int64_t i : indices)
    if (i < 0 || i >= total_) throw std::out_of_range("sampler index out of range");
  std::unique_lock<std::mutex> g(mu_);
  ++gen_;  // workers drop batches of the previous generation
  cv_slot_.wait(g, [this] { return busy_ == 0; });
  indices_ = indices;
  epoch_ = epoch;
  const int64_t n = (int64_t)indices_.size();
  nbatches_ = cfg_.drop_last ? n / cfg_.batch : (n + cfg_.batch - 1) / cfg_.batch;
  next_produce_ = 0;
  next_consume_ = 0;
  std::fill(slot_batch_.begin(), slot_batch_.end(), -1);
  g.unlock();
  cv_work_.notify_all();
}

// TrivialAugmentWide of one stored image (csrc/common/augment.hpp) with plain loops; the kernel
// record_augment writes the same bytes.
const uint8_t* RecordLoader::augmented(const uint8_t* img, int64_t gi, int64_t epoch,
                                       std::vector<uint8_t>& tmp) const {
  namespace aug = mipipe_aug;
  if (!augment_) return img;
  const int C = cfg_.C, H = cfg_.H, W = cfg_.W;
  const size_t plane = (size_t)H * W;
  tmp.resize((size_t)C * plane);
  uint8_t* out = tmp.data();
  const aug::Params par =
      aug::ta_wide_params(aug::sample_word(cfg_.seed, (uint64_t)epoch, (uint64_t)gi), -1);
  const int kind = aug::op_kind(par.op, C);
  if (kind == aug::kLut) {
    uint8_t lut[3][256];
    if (par.op == aug::kAutoContrast || par.op == aug::kEqualize) {
      for (int c = 0; c < C; ++c) {
        uint32_t hist[256] = {0};
        for (size_t p = 0; p < plane; ++p) ++hist[img[c * plane + p]];
        aug::hist_lut(par.op, hist, lut[c]);
      }
    } else {
      int mean = 0;
      if (par.op == aug::kContrast) {
        uint64_t sum = 0;
        for (size_t p = 0; p < plane; ++p)
          sum += (uint64_t)(C == 3 ? aug::grey(img[p], img[plane + p], img[2 * plane + p])
                                   : (int)img[p]);
        mean = aug::contrast_mean(sum, plane);
      }
      for (int v = 0; v < 256; ++v) {
        const uint8_t t = (uint8_t)aug::point_lut(par, mean, v);
        for (int c = 0; c < C; ++c) lut[c][v] = t;
      }
    }
    for (int c = 0; c < C; ++c)
      for (size_t p = 0; p < plane; ++p) out[c * plane + p] = lut[c][img[c * plane + p]];
  } else if (kind == aug::kColorBlend) {
    const int fq = aug::factor_q16(par);
    for (size_t p = 0; p < plane; ++p) {
      const int g = aug::grey(img[p], img[plane + p], img[2 * plane + p]);
      for (int c = 0; c < 3; ++c)
        out[c * plane + p] = (uint8_t)aug::blend(g, img[c * plane + p], fq);
    }
  } else if (kind == aug::kStencil) {
    const int fq = aug::factor_q16(par);
    for (int c = 0; c < C; ++c)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
          out[c * plane + (size_t)y * W + x] =
              (uint8_t)aug::sharpen(img + c * plane, y, x, H, W, fq);
  } else {
    const aug::Affine a = aug::affine_of(par);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        int ys = 0, xs = 0;
        const bool in = aug::affine_src(a, y, x, H, W, &ys, &xs);
        for (int c = 0; c < C; ++c)
          out[c * plane + (size_t)y * W + x] = in ? img[c * plane + (size_t)ys * W + xs] : 0;
      }
  }
  return out;
}

// Random Erasing on one sample of the output, [C][Ho][Wo] floats: the box becomes 0.0
void RecordLoader::erase(float* xs, int64_t gi, int64_t epoch, int Ho, int Wo) const {
  namespace aug = mipipe_aug;
  if (!cfg_.erase_pq) return;
  const aug::EraseBox b = aug::erase_box(
      aug::sample_word(cfg_.seed, (uint64_t)epoch, (uint64_t)gi), cfg_.erase_pq, Ho, Wo);
  for (int c = 0; c < cfg_.C; ++c)
    for (int y = b.y0; y < b.y0 + b.h; ++y)
      for (int x = b.x0; x < b.x0 + b.w; ++x) xs[((size_t)c * Ho + y) * Wo + x] = 0.f;
}

void RecordLoader::fill(int slot, int64_t b, const std::vector<int64_t>& idx, int64_t epoch) {
  const int C = cfg_.C, H = cfg_.H, W = cfg_.W, P = cfg_.pad;
  const int64_t i0 = b * cfg_.batch;
  const int n = (int)std::min<int64_t>(cfg_.batch, (int64_t)idx.size() - i0);
  float* xo = slot_x_[slot].data();
  int64_t* yo = slot_y_[slot].data();
  const size_t plane = (size_t)H * W;
  std::vector<uint8_t> tmp;
  for (int s = 0; s < n; ++s) {
    const int64_t gi = idx[i0 + s];
    const uint8_t* r = record(gi);
    int64_t label = 0;
    for (int k = 0; k < cfg_.label_bytes; ++k) label |= (int64_t)r[k] << (8 * k);
    yo[s] = label;
    const uint8_t* img = augmented(r + cfg_.label_bytes, gi, epoch, tmp);
    int dy = 0, dx = 0;
    bool flip = false;
    if (cfg_.train) {
      uint64_t h = splitmix64(cfg_.seed ^ splitmix64((uint64_t)epoch * 0x100000001b3ull ^ (uint64_t)gi));
      if (P > 0) {
        dy = (int)(h % (uint64_t)(2 * P + 1)) - P;
        dx = (int)((h >> 16) % (uint64_t)(2 * P + 1)) - P;
      }
      flip = cfg_.flip && ((h >> 40) & 1);
    }
    float* xs = xo + (size_t)s * C * plane;
    for (int c = 0; c < C; ++c) {
      const float sc = 1.f / (255.f * cfg_.stdv[c]);
      const float off = -cfg_.mean[c] / cfg_.stdv[c];
      const uint8_t* ip = img + (size_t)c * plane;
      float* op = xs + (size_t)c * plane;
      for (int y = 0; y < H; ++y) {
        const int sy = y + dy;
        for (int x = 0; x < W; ++x) {
          const int xx = flip ? W - 1 - x : x;
          const int sx = xx + dx;
          // zero padding (RandomCrop(padding=P) pads the uint8 image with 0)
          const float v = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? (float)ip[sy * W + sx] : 0.f;
          op[y * W + x] = v * sc + off;
        }
      }
    }
    erase(xs, gi, epoch, H, W);
  }
  slot_n_[slot] = n;
}

// "rrc": the box of rrc_box() resampled bilinearly to out_h x out_w, flipped, normalised.  The
// horizontal blend (8-bit pixels, Q16 weights) is exact in fp32; the vertical one is two rounded
// multiplies and a rounded add, then v * sc + off as in fill() — the NumPy definition
// (records.py reference_transform_rrc) and records.hip produce the same bits.
void RecordLoader::fill_rrc(int slot, int64_t b, const std::vector<int64_t>& idx, int64_t epoch) {
  namespace rrc = mipipe_rrc;
  const int C = cfg_.C, H = cfg_.H, W = cfg_.W, Ho = cfg_.out_h, Wo = cfg_.out_w;
  const int64_t i0 = b * cfg_.batch;
  const int n = (int)std::min<int64_t>(cfg_.batch, (int64_t)idx.size() - i0);
  float* xo = slot_x_[slot].data();
  int64_t* yo = slot_y_[slot].data();
  const size_t plane = (size_t)H * W, oplane = (size_t)Ho * Wo;
  // the column taps of one sample, the flip folded in: source columns and their weights
  std::vector<int> cx0(Wo), cx1(Wo);
  std::vector<float> lx0(Wo), lx1(Wo);
  std::vector<uint8_t> tmp;
  for (int s = 0; s < n; ++s) {
    const int64_t gi = idx[i0 + s];
    const uint8_t* r = record(gi);
    int64_t label = 0;
    for (int k = 0; k < cfg_.label_bytes; ++k) label |= (int64_t)r[k] << (8 * k);
    yo[s] = label;
    const uint8_t* img = augmented(r + cfg_.label_bytes, gi, epoch, tmp);
    const rrc::Box bx = rrc::rrc_box(cfg_.seed, (uint64_t)epoch, (uint64_t)gi, H, W, cfg_.train,
                                     cfg_.flip);
    for (int x = 0; x < Wo; ++x) {
      const rrc::Tap t = rrc::rrc_tap(bx.flip ? Wo - 1 - x : x, bx.w, Wo);
      cx0[x] = bx.x0 + t.i0;
      cx1[x] = bx.x0 + t.i1;
      lx1[x] = (float)t.frac * (1.f / 65536.f);
      lx0[x] = 1.f - lx1[x];
    }
    float* xs = xo + (size_t)s * C * oplane;
    for (int y = 0; y < Ho; ++y) {
      const rrc::Tap t = rrc::rrc_tap(y, bx.h, Ho);
      const float ly1 = (float)t.frac * (1.f / 65536.f), ly0 = 1.f - ly1;
      for (int c = 0; c < C; ++c) {
        const float sc = 1.f / (255.f * cfg_.stdv[c]);
        const float off = -cfg_.mean[c] / cfg_.stdv[c];
        const uint8_t* r0 = img + (size_t)c * plane + (size_t)(bx.y0 + t.i0) * W;
        const uint8_t* r1 = img + (size_t)c * plane + (size_t)(bx.y0 + t.i1) * W;
        float* op = xs + (size_t)c * oplane + (size_t)y * Wo;
        for (int x = 0; x < Wo; ++x) {
          const float top = (float)r0[cx0[x]] * lx0[x] + (float)r0[cx1[x]] * lx1[x];
          const float bot = (float)r1[cx0[x]] * lx0[x] + (float)r1[cx1[x]] * lx1[x];
          const float ta = top * ly0, tb = bot * ly1;
          const float v = ta + tb;
          op[x] = v * sc + off;
        }
      }
    }
    erase(xs, gi, epoch, Ho, Wo);
  }
  slot_n_[slot] = n;
}

// raw mode: gather only — whole records (label bytes included) and their global indices
void RecordLoader::fill_raw(int slot, int64_t b, const std::vector<int64_t>& idx) {
  const int64_t i0 = b * cfg_.batch;
  const int n = (int)std::min<int64_t>(cfg_.batch, (int64_t)idx.size() - i0);
  uint8_t* ro = slot_raw_[slot].data();
  int64_t* io = slot_y_[slot].data();
  for (int s = 0; s < n; ++s) {
    const int64_t gi = idx[i0 + s];
    memcpy(ro + (size_t)s * rec_bytes_, record(gi), rec_bytes_);
    io[s] = gi;
  }
  slot_n_[slot] = n;
}

void RecordLoader::worker() {
  std::unique_lock<std::mutex> g(mu_);
  while (true) {
    cv_work_.wait(g, [this] {
      return shutdown_ || (next_produce_ < nbatches_ && next_produce_ - next_consume_ < cfg_.prefetch);
    });
    if (shutdown_) return;
    const int64_t b = next_produce_++;
    const int slot = (int)(b % cfg_.prefetch);
    const uint64_t gen = gen_;
    const std::vector<int64_t>* idx = &indices_;
    const int64_t epoch = epoch_;
    ++busy_;
    g.unlock();
    if (cfg_.raw) fill_raw(slot, b, *idx);
    else if (rrc_) fill_rrc(slot, b, *idx, epoch);
    else fill(slot, b, *idx, epoch);
    g.lock();
    --busy_;
    if (gen == gen_) slot_batch_[slot] = b;
    cv_slot_.notify_all();
  }
}

int RecordLoader::next(float* x, int64_t* y) {
  if (cfg_.raw) throw std::logic_error("next on a raw-mode loader (use next_raw)");
  std::unique_lock<std::mutex> g(mu_);
  if (next_consume_ >= nbatches_) return 0;
  const int64_t b = next_consume_;
  const int slot = (int)(b % cfg_.prefetch);
  cv_slot_.wait(g, [&] { return slot_batch_[slot] == b || shutdown_; });
  if (shutdown_) return 0;
  const int n = slot_n_[slot];
  g.unlock();
  memcpy(x, slot_x_[slot].data(), (size_t)n * out_per_ * sizeof(float));
  memcpy(y, slot_y_[slot].data(), (size_t)n * sizeof(int64_t));
  g.lock();
  slot_batch_[slot] = -1;
  ++next_consume_;
  g.unlock();
  cv_work_.notify_all();
  return n;
}

int RecordLoader::next_raw(uint8_t* rec, int64_t* idx) {
  if (!cfg_.raw) throw std::logic_error("next_raw needs LoaderConfig::raw");
  std::unique_lock<std::mutex> g(mu_);
  if (next_consume_ >= nbatches_) return 0;
  const int64_t b = next_consume_;
  const int slot = (int)(b % cfg_.prefetch);
  cv_slot_.wait(g, [&] { return slot_batch_[slot] == b || shutdown_; });
  if (shutdown_) return 0;
  const int n = slot_n_[slot];
  g.unlock();
  memcpy(rec, slot_raw_[slot].data(), (size_t)n * rec_bytes_);
  memcpy(idx, slot_y_[slot].data(), (size_t)n * sizeof(int64_t));
  g.lock();
  slot_batch_[slot] = -1;
  ++next_consume_;
  g.unlock();
  cv_work_.notify_all();
  return n;
}

int64_t RecordLoader::batches_per_epoch() const { return nbatches_; }

}  // namespace mipipe_rt
