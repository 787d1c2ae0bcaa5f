// zstd_walk_cli -- cloudini_amd/csrc/zstd_decode_walk.h on the CPU, for tests/test_zstd_walk_cpu.py (built there with
// -fsanitize=address,undefined). Every frame is copied into a heap block of exactly its size, so a read outside the span is
// the sanitizer's to find.
//   input  file: [u32 cases] then per case [u32 bytes][u32 capacity][frame]
//   output: per case one line "verdict n_recs total" and per record "kind src size out regen streams tree desc log n_sym weights(hex)"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zstd_decode_walk.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t cases = 0;
  if (fread(&cases, 4, 1, f) != 1) return 2;
  for (uint32_t c = 0; c < cases; ++c) {
    uint32_t head[2];
    if (fread(head, 4, 2, f) != 2) return 2;
    uint8_t* frame = (uint8_t*)malloc(head[0] ? head[0] : 1);
    if (head[0] && fread(frame, 1, head[0], f) != head[0]) return 2;
    // the counting pass, then the full one with exactly the room the count asks for (what the walk kernel does)
    cldn::ZdFse t;
    uint32_t counted = 0, total = 0;
    (void)cldn::zd_walk(head[0] ? frame : nullptr, head[0], head[1], nullptr, 0, nullptr, &t, &counted, &total);
    std::vector<cldn::ZdBlock> recs(counted ? counted : 1);
    uint8_t* weights = (uint8_t*)malloc((size_t)(counted ? counted : 1) * 256);
    memset(weights, 0, (size_t)(counted ? counted : 1) * 256);
    uint32_t n = 0;
    const uint32_t v = cldn::zd_walk(head[0] ? frame : nullptr, head[0], head[1], recs.data(), counted, weights, &t, &n, &total);
    if (n > counted) return 3;
    printf("%u %u %u\n", v, n, total);
    for (uint32_t i = 0; i < n; ++i) {
      const cldn::ZdBlock& r = recs[i];
      printf("%u %u %u %u %u %u %u %u %u %u ", r.kind, r.src, r.size, r.out, r.regen, r.streams, r.tree, r.desc, r.log, r.n_sym);
      for (uint32_t k = 0; k < r.n_sym; ++k) printf("%02x", weights[256 * (size_t)i + k]);
      printf("\n");
    }
    free(weights);
    free(frame);
  }
  fclose(f);
  return 0;
}
