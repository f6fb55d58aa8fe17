// The plan integer of the conv / GEMM dispatch: one int per (op, shape) in tune tables, tests and
// the Python API.  This header is the only place that knows its encoding.  Host-only and free of
// HIP / torch includes (tools/plan_dump.cpp builds it with the system compiler).
//
//   plan = tile id + kPlanSplit * split count  [| kPlanWs]
//
// Two readings of the same layout:
//  * conv forward, inference forward, forward-style data-grad (decode_conv_plan): a split count
//    >= 2 runs the k-steps in that many slices into an fp32 workspace summed in slice order;
//    a bare tile id (or a negative plan: the heuristic tile) does not split.
//  * conv weight-grad, gemm, gemm_gelu (decode_gemm_plan): a split count of 0 is the heuristic
//    split (-1), and kPlanWs sends the split partials through per-split workspace slices summed
//    in order instead of fp32 atomics.
// Both decoders are total: every integer decodes as it always has, so a table from elsewhere
// keeps doing what it did.
#pragma once

namespace mipipe {

constexpr int kPlanSplit = 16;
constexpr int kPlanWs = 1024;
constexpr int kPlanLegacyLibrary = 4096;  // round-3 tables' library plans: the heuristic now

struct Plan {
  int tile;    // tile config id; negative: the heuristic
  int splits;  // conv plans: >= 1.  gemm plans: > 0 forces the count, -1 = heuristic
  bool ws;     // gemm plans only: split partials through workspace slices
};

// (the workspace bit is not part of a conv plan: it reads as split count)
inline Plan decode_conv_plan(int p) {
  if (p < kPlanSplit) return {p, 1, false};
  return {p % kPlanSplit, p / kPlanSplit, false};
}
inline int encode_conv_plan(int tile, int splits) {
  return splits > 1 ? tile + kPlanSplit * splits : tile;
}

// legacy_library (gemm, gemm_gelu; not the weight-grad): plans >= kPlanLegacyLibrary are heuristic
inline Plan decode_gemm_plan(int p, bool legacy_library) {
  if (legacy_library && p >= kPlanLegacyLibrary) p = -1;
  if (p < 0) return {-1, -1, false};
  const bool ws = (p & kPlanWs) != 0;
  p &= ~kPlanWs;
  const int sp = p / kPlanSplit;
  return {p % kPlanSplit, sp > 0 ? sp : -1, ws};
}
// sp <= 0: the heuristic split (field 0), so a decoded Plan encodes back to its integer
inline int encode_gemm_plan(int tile, int sp, bool ws) {
  return (tile + kPlanSplit * (sp > 0 ? sp : 0)) | (ws ? kPlanWs : 0);
}

// what a tune-table entry may hold: -1 (erase) or a plan whose tile field names a tile config
inline bool plan_id_ok(int p, int n_tiles) { return p == -1 || (p >= 0 && p % kPlanSplit < n_tiles); }

}  // namespace mipipe
