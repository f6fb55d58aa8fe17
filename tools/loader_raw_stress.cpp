// Stand-alone stress program for the record loader's raw mode (csrc/runtime/loader.cpp), meant
// to be built with a host sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=thread -Icsrc/runtime tools/loader_raw_stress.cpp \
//       csrc/runtime/loader.cpp -o loader_raw_stress_tsan -lpthread
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined ... (same)
// It writes two record files, then drives a raw-mode loader with several workers through
// start_epoch generations — complete epochs, an epoch abandoned half way (the next generation
// starts while workers are still filling slots) and a partial last batch — and checks every
// byte and index that next_raw returns.  A last section drives the host "rrc" transform
// (fill_rrc: float slots sized for the output, not the stored shape) the same way, down- and
// up-scaling, and checks every value against the taps of common/rrc.hpp.  The augmenting host
// path comes last (LoaderConfig::auto_augment / erase_pq: TrivialAugmentWide's gathers and stencil
// on odd, one-channel and 2x2 images, Random Erasing on the output): the crop transform's values
// are checked against a per-pixel recomputation from common/augment.hpp, the rrc transform's
// against their range.
// Exit status 0 = all checks passed.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "../common/augment.hpp"
#include "../common/rrc.hpp"
#include "runtime.hpp"

using namespace mipipe_rt;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

static uint8_t byte_of(int64_t rec, size_t k) { return (uint8_t)((rec * 131 + (int64_t)k * 7 + 3) & 0xFF); }

static std::string write_file(int64_t first, int64_t count, size_t rec_bytes) {
  char path[] = "/tmp/loader_raw_stress_XXXXXX";
  int fd = mkstemp(path);
  if (fd < 0) { std::perror("mkstemp"); std::exit(2); }
  std::vector<uint8_t> buf((size_t)count * rec_bytes);
  for (int64_t r = 0; r < count; ++r)
    for (size_t k = 0; k < rec_bytes; ++k) buf[(size_t)r * rec_bytes + k] = byte_of(first + r, k);
  if (write(fd, buf.data(), buf.size()) != (ssize_t)buf.size()) { std::perror("write"); std::exit(2); }
  close(fd);
  return path;
}

// consume up to max_batches batches (< 0: the whole epoch); returns the samples seen
static int64_t consume(RecordLoader& ld, const std::vector<int64_t>& order, int batch,
                       size_t rec_bytes, int max_batches) {
  std::vector<uint8_t> rec((size_t)batch * rec_bytes);
  std::vector<int64_t> idx(batch);
  int64_t seen = 0;
  for (int b = 0; max_batches < 0 || b < max_batches; ++b) {
    const int n = ld.next_raw(rec.data(), idx.data());
    if (n == 0) break;
    CHECK(n == (int)std::min<int64_t>(batch, (int64_t)order.size() - seen));
    for (int s = 0; s < n; ++s) {
      const int64_t gi = order[seen + s];
      CHECK(idx[s] == gi);
      for (size_t k = 0; k < rec_bytes; ++k)
        if (rec[(size_t)s * rec_bytes + k] != byte_of(gi, k)) {
          CHECK(!"record byte mismatch");
          break;
        }
    }
    seen += n;
  }
  return seen;
}

// the rrc value of one output element, recomputed from the definition (mean 0, std 1)
static float rrc_value(int64_t gi, int c, int oy, int ox, int H, int W, int Ho, int Wo,
                       size_t label_bytes, uint64_t seed, uint64_t epoch, bool train) {
  const mipipe_rrc::Box bx = mipipe_rrc::rrc_box(seed, epoch, (uint64_t)gi, H, W, train, train);
  const mipipe_rrc::Tap ty = mipipe_rrc::rrc_tap(oy, bx.h, Ho);
  const mipipe_rrc::Tap tx = mipipe_rrc::rrc_tap(bx.flip ? Wo - 1 - ox : ox, bx.w, Wo);
  auto px = [&](int y, int x) {
    return (float)byte_of(gi, label_bytes + ((size_t)c * H + (bx.y0 + y)) * W + (bx.x0 + x));
  };
  const float lx1 = (float)tx.frac / 65536.f, lx0 = 1.f - lx1;
  const float ly1 = (float)ty.frac / 65536.f, ly0 = 1.f - ly1;
  const float top = px(ty.i0, tx.i0) * lx0 + px(ty.i0, tx.i1) * lx1;
  const float bot = px(ty.i1, tx.i0) * lx0 + px(ty.i1, tx.i1) * lx1;
  const float a = top * ly0, b = bot * ly1;
  return (a + b) * (1.f / 255.f);
}

static void rrc_section(LoaderConfig cfg, int Ho, int Wo, bool train, int64_t total) {
  cfg.raw = false;
  cfg.train = train;
  cfg.flip = train;
  cfg.transform = "rrc";
  cfg.out_h = Ho;
  cfg.out_w = Wo;
  cfg.seed = 11;
  RecordLoader ld(cfg);
  const size_t per = (size_t)cfg.C * Ho * Wo;
  std::vector<float> x((size_t)cfg.batch * per);
  std::vector<int64_t> y(cfg.batch);
  std::vector<int64_t> order(total);
  std::iota(order.begin(), order.end(), 0);
  for (int round = 0; round < 12; ++round) {
    for (int64_t i = total - 1; i > 0; --i) std::swap(order[i], order[(i * 7919 + round * 31) % (i + 1)]);
    ld.start_epoch(order, round);
    int64_t seen = 0;
    for (int b = 0; round % 3 != 1 || b < 2; ++b) {  // every third epoch is abandoned mid-way
      const int n = ld.next(x.data(), y.data());
      if (n == 0) break;
      for (int s = 0; s < n; ++s) {
        const int64_t gi = order[seen + s];
        int64_t label = 0;
        for (int k = 0; k < cfg.label_bytes; ++k) label |= (int64_t)byte_of(gi, k) << (8 * k);
        CHECK(y[s] == label);
        for (int c = 0; c < cfg.C; ++c)
          for (int oy = 0; oy < Ho; ++oy)
            for (int ox = 0; ox < Wo; ++ox) {
              const float want = rrc_value(gi, c, oy, ox, cfg.H, cfg.W, Ho, Wo, cfg.label_bytes,
                                           cfg.seed, (uint64_t)round, train);
              if (x[(size_t)s * per + ((size_t)c * Ho + oy) * Wo + ox] != want) {
                CHECK(!"rrc value mismatch");
                ox = Wo; oy = Ho; c = cfg.C;
              }
            }
      }
      seen += n;
    }
    CHECK(round % 3 == 1 ? seen == 2 * cfg.batch : seen == total);
  }
  ld.start_epoch(order, 100);  // destroyed with workers busy
}

// TrivialAugmentWide of record gi, pixel by pixel from the definitions (no tables): the loader's
// augmented() must give the same bytes
static std::vector<uint8_t> augment_ref(int64_t gi, uint64_t seed, uint64_t epoch, int C, int H,
                                        int W, size_t label_bytes) {
  namespace aug = mipipe_aug;
  const size_t plane = (size_t)H * W;
  std::vector<uint8_t> src(C * plane), out(C * plane);
  for (size_t k = 0; k < src.size(); ++k) src[k] = byte_of(gi, label_bytes + k);
  const aug::Params par = aug::ta_wide_params(aug::sample_word(seed, epoch, (uint64_t)gi), -1);
  const int fq = aug::factor_q16(par);
  auto px = [&](int c, size_t p) { return (int)src[c * plane + p]; };
  auto grey = [&](size_t p) { return C == 3 ? aug::grey(px(0, p), px(1, p), px(2, p)) : px(0, p); };
  uint64_t gsum = 0;
  for (size_t p = 0; p < plane; ++p) gsum += (uint64_t)grey(p);
  const aug::Affine a = aug::affine_of(par);
  for (int c = 0; c < C; ++c) {
    uint32_t hist[256] = {0};
    for (size_t p = 0; p < plane; ++p) ++hist[px(c, p)];
    uint8_t lut[256];
    if (par.op == aug::kAutoContrast || par.op == aug::kEqualize) aug::hist_lut(par.op, hist, lut);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t p = (size_t)y * W + x;
        const int v = px(c, p);
        int r = v;
        switch (par.op) {
          case aug::kShearX: case aug::kShearY: case aug::kTranslateX: case aug::kTranslateY:
          case aug::kRotate: {
            int ys, xs;
            r = aug::affine_src(a, y, x, H, W, &ys, &xs) ? px(c, (size_t)ys * W + xs) : 0;
            break;
          }
          case aug::kColor: r = C == 3 ? aug::blend(grey(p), v, fq) : v; break;
          case aug::kSharpness: r = aug::sharpen(src.data() + c * plane, y, x, H, W, fq); break;
          case aug::kAutoContrast: case aug::kEqualize: r = lut[v]; break;
          default: r = aug::point_lut(par, aug::contrast_mean(gsum, plane), v); break;
        }
        out[c * plane + p] = (uint8_t)r;
      }
  }
  return out;
}

static void augment_section(int C, int H, int W, int Ho, int Wo, bool rrc) {
  const int label_bytes = 2, batch = 5;
  const size_t rec_bytes = label_bytes + (size_t)C * H * W;
  const int64_t n0 = 40, n1 = 27, total = n0 + n1;
  LoaderConfig cfg;
  cfg.files = {write_file(0, n0, rec_bytes), write_file(n0, n1, rec_bytes)};
  cfg.label_bytes = label_bytes;
  cfg.C = C; cfg.H = H; cfg.W = W;
  cfg.batch = batch;
  cfg.mean.assign(C, 0.f);
  cfg.stdv.assign(C, 1.f);
  cfg.workers = 6;
  cfg.prefetch = 3;
  cfg.pad = 0;
  cfg.flip = false;
  cfg.seed = 1234;
  cfg.auto_augment = "ta_wide";
  cfg.erase_pq = 1u << 23;
  if (rrc) {
    cfg.transform = "rrc";
    cfg.out_h = Ho;
    cfg.out_w = Wo;
  }
  {
    RecordLoader ld(cfg);
    const size_t per = (size_t)C * Ho * Wo;
    std::vector<float> x((size_t)batch * per);
    std::vector<int64_t> y(batch);
    std::vector<int64_t> order(total);
    std::iota(order.begin(), order.end(), 0);
    int ops_seen = 0, erased = 0;
    for (int round = 0; round < 9; ++round) {
      for (int64_t i = total - 1; i > 0; --i) std::swap(order[i], order[(i * 7919 + round * 31) % (i + 1)]);
      ld.start_epoch(order, round);
      int64_t seen = 0;
      for (int b = 0; round % 3 != 1 || b < 2; ++b) {  // every third epoch is abandoned mid-way
        const int n = ld.next(x.data(), y.data());
        if (n == 0) break;
        for (int s = 0; s < n; ++s) {
          const int64_t gi = order[seen + s];
          int64_t label = 0;
          for (int k = 0; k < label_bytes; ++k) label |= (int64_t)byte_of(gi, k) << (8 * k);
          CHECK(y[s] == label);
          const uint64_t h0 = mipipe_aug::sample_word(cfg.seed, (uint64_t)round, (uint64_t)gi);
          ops_seen |= 1 << mipipe_aug::ta_wide_params(h0, -1).op;
          const mipipe_aug::EraseBox bx = mipipe_aug::erase_box(h0, cfg.erase_pq, Ho, Wo);
          erased += bx.h > 0;
          std::vector<uint8_t> want;
          if (!rrc) want = augment_ref(gi, cfg.seed, (uint64_t)round, C, H, W, label_bytes);
          for (int c = 0; c < C; ++c)
            for (int oy = 0; oy < Ho; ++oy)
              for (int ox = 0; ox < Wo; ++ox) {
                const float v = x[(size_t)s * per + ((size_t)c * Ho + oy) * Wo + ox];
                const bool in_box = oy >= bx.y0 && oy < bx.y0 + bx.h && ox >= bx.x0 && ox < bx.x0 + bx.w;
                bool ok = v >= 0.f && v <= 1.f;
                if (in_box) ok = v == 0.f;
                else if (!rrc) ok = v == (float)want[((size_t)c * H + oy) * W + ox] * (1.f / 255.f);
                if (!ok) {
                  CHECK(!"augmented value mismatch");
                  ox = Wo; oy = Ho; c = C;
                }
              }
        }
        seen += n;
      }
      CHECK(round % 3 == 1 ? seen == 2 * batch : seen == total);
    }
    CHECK(ops_seen == (1 << mipipe_aug::kOps) - 1);  // every op ran
    CHECK(erased > 0 || Ho * Wo < 16);  // no box fits strictly inside a 2x2 output
    ld.start_epoch(order, 100);  // destroyed with workers busy
  }
  for (auto& f : cfg.files) unlink(f.c_str());
}

int main() {
  const int C = 3, H = 8, W = 8, label_bytes = 2, batch = 5;
  const size_t rec_bytes = label_bytes + (size_t)C * H * W;
  const int64_t n0 = 20, n1 = 17, total = n0 + n1;
  LoaderConfig cfg;
  cfg.files = {write_file(0, n0, rec_bytes), write_file(n0, n1, rec_bytes)};
  cfg.label_bytes = label_bytes;
  cfg.C = C; cfg.H = H; cfg.W = W;
  cfg.batch = batch;
  cfg.mean = {0.f, 0.f, 0.f};
  cfg.stdv = {1.f, 1.f, 1.f};
  cfg.workers = 6;
  cfg.prefetch = 3;
  cfg.raw = true;
  {
    RecordLoader ld(cfg);
    CHECK(ld.size() == total);
    CHECK(ld.record_bytes() == rec_bytes);
    std::vector<int64_t> order(total);
    std::iota(order.begin(), order.end(), 0);
    for (int round = 0; round < 40; ++round) {
      // a different permutation every generation
      for (int64_t i = total - 1; i > 0; --i) std::swap(order[i], order[(i * 7919 + round * 31) % (i + 1)]);
      ld.start_epoch(order, round);
      CHECK(ld.batches_per_epoch() == (total + batch - 1) / batch);
      if (round % 3 == 1) {
        // abandon this epoch after two batches: the next start_epoch arrives mid-epoch
        CHECK(consume(ld, order, batch, rec_bytes, 2) == 2 * batch);
        continue;
      }
      if (round % 3 == 2) continue;  // a generation nobody consumes at all
      CHECK(consume(ld, order, batch, rec_bytes, -1) == total);
      std::vector<uint8_t> r(batch * rec_bytes);
      std::vector<int64_t> ix(batch);
      CHECK(ld.next_raw(r.data(), ix.data()) == 0);  // exhausted
    }
    // a rank's shard (odd samples, drop_last off) started right after a half-consumed epoch
    std::vector<int64_t> shard;
    for (int64_t i = 1; i < total; i += 2) shard.push_back(i);
    ld.start_epoch(order, 100);
    consume(ld, order, batch, rec_bytes, 1);
    ld.start_epoch(shard, 101);
    CHECK(consume(ld, shard, batch, rec_bytes, -1) == (int64_t)shard.size());
    ld.start_epoch(order, 102);  // destroyed with workers busy
  }
  {
    LoaderConfig c2 = cfg;
    c2.drop_last = true;
    RecordLoader ld(c2);
    std::vector<int64_t> order(total);
    std::iota(order.begin(), order.end(), 0);
    ld.start_epoch(order, 0);
    CHECK(ld.batches_per_epoch() == total / batch);
    CHECK(consume(ld, order, batch, rec_bytes, -1) == (total / batch) * batch);
  }
  rrc_section(cfg, 5, 7, true, total);    // 8x8 boxes down and up to odd extents
  rrc_section(cfg, 19, 13, true, total);  // output larger than the stored image
  rrc_section(cfg, 6, 6, false, total);   // evaluation: centre 7x7 -> 6x6
  augment_section(3, 8, 8, 8, 8, false);
  augment_section(3, 7, 11, 7, 11, false);  // odd extents, an odd record stride
  augment_section(1, 9, 5, 9, 5, false);    // one channel: Color is the identity
  augment_section(3, 2, 2, 2, 2, false);    // no interior pixel for the stencil
  augment_section(3, 7, 11, 5, 9, true);    // augment -> rrc -> erase
  augment_section(1, 9, 5, 12, 3, true);
  for (auto& f : cfg.files) unlink(f.c_str());
  std::printf(g_fail ? "loader_raw_stress: %d check(s) FAILED\n" : "loader_raw_stress: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
