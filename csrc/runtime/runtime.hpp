// mipipe native runtime (module ``mipipe._runtime``): process-group supervisor, DAG scheduler
// core and multi-threaded record loader.  Host C++ only (no GPU code), bound in bindings.cpp.
#pragma once
#include <sys/types.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace mipipe_rt {

// ---------------------------------------------------------------- process supervisor
class ProcessGroup {
 public:
  explicit ProcessGroup(bool echo) : echo_(echo) {}
  ~ProcessGroup();
  // argv[0] is looked up on PATH; env as "K=V" strings (empty: inherit); returns child index
  int spawn(const std::vector<std::string>& argv, const std::vector<std::string>& env,
            const std::string& cwd, const std::string& log_path, const std::string& prefix);
  int wait(double timeout, double grace);
  void signal_all(int sig);
  void interrupt() { interrupted_ = true; }
  std::vector<int> exit_codes() const;
  std::vector<int> pids() const;
  int failed_rank() const { return failed_rank_; }

 private:
  struct Child {
    pid_t pid = -1;
    int out_fd = -1;
    FILE* log = nullptr;
    std::string prefix;
    bool exited = false;
    int code = -1;
  };
  void pump_loop();
  bool reap_nonblocking();
  void reap_all_blocking();
  bool echo_;
  std::vector<Child> children_;
  std::mutex mu_;
  std::thread pump_;
  std::atomic<bool> stop_pump_{false}, all_spawned_{false}, interrupted_{false};
  bool finished_ = false;
  int failed_rank_ = -1;
};

// ---------------------------------------------------------------- DAG scheduler core
class DagScheduler {
 public:
  enum State { kPending = 0, kRunning = 1, kSucceeded = 2, kCached = 3, kSkipped = 4,
               kFailed = 5, kCancelled = 6 };
  DagScheduler(int n, const std::vector<std::vector<int>>& deps,
               const std::vector<bool>& always_run, bool fail_fast);
  std::vector<int> next_ready();
  void complete(int i, int state);
  std::vector<int> take_cancelled();
  // a failure outside this DAG (fail-fast across sub-DAGs): cancel pending non-exit tasks
  void mark_external_failure() { any_failed_ = true; }
  bool finished() const;
  bool deadlocked() const;
  const std::vector<int>& states() const { return state_; }
  const std::vector<int>& topo_order() const { return topo_; }

 private:
  int n_;
  std::vector<std::vector<int>> deps_;
  std::vector<bool> always_;
  bool fail_fast_;
  std::vector<int> state_;
  std::vector<std::vector<int>> children_;
  std::vector<int> topo_, cancelled_;
  int running_ = 0;
  bool any_failed_ = false;
};

// ---------------------------------------------------------------- record loader
struct LoaderConfig {
  std::vector<std::string> files;
  int header_bytes = 0;
  int label_bytes = 1;
  int C = 3, H = 32, W = 32;
  int batch = 128;
  bool train = true;
  int pad = 4;
  bool flip = true;
  std::vector<float> mean, stdv;
  uint64_t seed = 0;
  int workers = 8;
  int prefetch = 4;
  bool drop_last = false;
  // raw mode: workers only gather whole records (label bytes included) and their global sample
  // indices; crop / flip / normalise run on the device (csrc/kernels/records.hip)
  bool raw = false;
  // "crop": RandomCrop(pad) + flip + Normalize at the stored size.  "rrc": RandomResizedCrop +
  // flip + Normalize (train) / 7/8 centre crop (eval), resized bilinearly to out_h x out_w
  // (0 = stored size); the geometry is csrc/common/rrc.hpp, pad is not used.
  std::string transform = "crop";
  int out_h = 0, out_w = 0;
  // Per-sample augmentation of the non-raw modes (csrc/common/augment.hpp; raw mode leaves both to
  // the device, csrc/kernels/augment.hip), training only.  auto_augment: "" or "ta_wide"
  // (TrivialAugmentWide on the stored image, before the transform; C must be 1 or 3).  erase_pq:
  // Random Erasing's probability as round(p * 2^24), the box zeroed in the transform's output.
  std::string auto_augment;
  uint32_t erase_pq = 0;
};

class RecordLoader {
 public:
  explicit RecordLoader(const LoaderConfig& cfg);
  ~RecordLoader();
  int64_t size() const { return total_; }
  void start_epoch(const std::vector<int64_t>& indices, int64_t epoch);
  // copies the next batch to x [n,C,H,W] f32 ("rrc": [n,C,out_h,out_w]) / y [n] i64; returns n
  // (0 = epoch exhausted)
  int next(float* x, int64_t* y);
  // raw mode: copies the next batch's records to rec [n, record_bytes] u8 and their global sample
  // indices to idx [n] i64; returns n (0 = epoch exhausted)
  int next_raw(uint8_t* rec, int64_t* idx);
  size_t record_bytes() const { return rec_bytes_; }
  int64_t batches_per_epoch() const;
  const uint8_t* record(int64_t i) const;

 private:
  void worker();
  void fill(int slot, int64_t b, const std::vector<int64_t>& idx, int64_t epoch);
  void fill_rrc(int slot, int64_t b, const std::vector<int64_t>& idx, int64_t epoch);
  void fill_raw(int slot, int64_t b, const std::vector<int64_t>& idx);
  // the image a transform reads: the stored one, or its augmentation written to tmp
  const uint8_t* augmented(const uint8_t* img, int64_t gi, int64_t epoch,
                           std::vector<uint8_t>& tmp) const;
  void erase(float* xs, int64_t gi, int64_t epoch, int Ho, int Wo) const;
  LoaderConfig cfg_;
  bool rrc_ = false;
  bool augment_ = false;
  size_t rec_bytes_ = 0;
  size_t out_per_ = 0;  // floats of one decoded sample
  std::vector<std::pair<const uint8_t*, size_t>> maps_;
  std::vector<int64_t> file_start_;
  int64_t total_ = 0;
  std::vector<std::vector<float>> slot_x_;
  std::vector<std::vector<int64_t>> slot_y_;  // labels; raw mode: sample indices
  std::vector<std::vector<uint8_t>> slot_raw_;
  std::vector<int> slot_n_;
  std::vector<int64_t> slot_batch_;
  std::vector<int64_t> indices_;
  int64_t epoch_ = 0, nbatches_ = 0, next_produce_ = 0, next_consume_ = 0;
  uint64_t gen_ = 0;
  int busy_ = 0;
  bool shutdown_ = false;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_slot_;
  std::vector<std::thread> threads_;
};

}  // namespace mipipe_rt
