// Host-side dump of the plan codec (csrc/kernels/plan.hpp).  For every plan integer p in
// [lo, hi] one line:
//   p | conv: tile splits | gemm: tile splits ws | gemm, legacy rule: tile splits ws |
//   plan_id_ok(p, n_tiles) | encode_conv(decode_conv(p)) | encode_gemm(decode_gemm(p))
// then one line "E tile sp ws encode_conv_plan(tile, sp) encode_gemm_plan(tile, sp, ws)" per
// tile in [0, n_tiles) and sp in [0, 32].  tests/test_plan_codec_cpu.py builds it with the
// system compiler and compares with the arithmetic written out in Python.
//   g++ -O1 -std=c++17 -Icsrc/kernels tools/plan_dump.cpp -o dump && ./dump -1 8191 15
#include <cstdio>
#include <cstdlib>

#include "plan.hpp"

int main(int argc, char** argv) {
  using namespace mipipe;
  const int lo = argc > 1 ? atoi(argv[1]) : -1;
  const int hi = argc > 2 ? atoi(argv[2]) : 8191;
  const int n_tiles = argc > 3 ? atoi(argv[3]) : 15;
  for (int p = lo; p <= hi; ++p) {
    const Plan c = decode_conv_plan(p), g = decode_gemm_plan(p, false), l = decode_gemm_plan(p, true);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", p, c.tile, c.splits, g.tile, g.splits, (int)g.ws,
           l.tile, l.splits, (int)l.ws, (int)plan_id_ok(p, n_tiles),
           encode_conv_plan(c.tile, c.splits), encode_gemm_plan(g.tile, g.splits, g.ws));
  }
  for (int t = 0; t < n_tiles; ++t)
    for (int sp = 0; sp <= 32; ++sp)
      for (int ws = 0; ws < 2; ++ws)
        printf("E %d %d %d %d %d\n", t, sp, ws, encode_conv_plan(t, sp), encode_gemm_plan(t, sp, ws != 0));
  return 0;
}
