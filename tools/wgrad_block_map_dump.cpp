// Host-side dump of splitk_block_map (csrc/kernels/block_map.hpp), the placement of split-K
// weight-grad blocks on a 1-D grid.  For every tiles in 1..T and splits in 1..S (in that nesting
// order) and every linear block id L in [0, tiles*splits), writes the mapped (tile, split) as two
// little-endian uint16 to stdout.  tests/test_wgrad_block_map_cpu.py builds it with the system
// compiler and checks the placement properties.
//   g++ -O1 -std=c++17 -Icsrc/kernels tools/wgrad_block_map_dump.cpp -o dump && ./dump 72 72
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "block_map.hpp"

int main(int argc, char** argv) {
  const uint32_t T = argc > 1 ? (uint32_t)atoi(argv[1]) : 72;
  const uint32_t S = argc > 2 ? (uint32_t)atoi(argv[2]) : 72;
  if (T < 1 || S < 1 || T * S > 65535) {
    fprintf(stderr, "usage: %s [max_tiles] [max_splits]  (product <= 65535)\n", argv[0]);
    return 2;
  }
  std::vector<uint16_t> buf;
  for (uint32_t tiles = 1; tiles <= T; ++tiles)
    for (uint32_t splits = 1; splits <= S; ++splits) {
      buf.clear();
      for (uint32_t L = 0; L < tiles * splits; ++L) {
        const mipipe::TileSplit m = mipipe::splitk_block_map(L, tiles, splits);
        buf.push_back((uint16_t)m.tile);
        buf.push_back((uint16_t)m.split);
        if (m.tile > 65535 || m.split > 65535) return 3;
      }
      if (fwrite(buf.data(), sizeof(uint16_t), buf.size(), stdout) != buf.size()) return 4;
    }
  return 0;
}
