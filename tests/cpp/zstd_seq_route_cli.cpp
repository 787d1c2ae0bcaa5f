// zstd_seq_route_cli -- the kernels cloudini_amd/csrc/stage1_decode_route.h lists for one XYZ float plan's ZSTD call without and
// with the fact zstd_seq (cldn_hip_codec_set_zstd_sequences), and for a ZSTD call without chunks with it. One row of kernel names
// each (tests/test_gpu_zstd_seq_decode.py).
#include <cstdio>
#include <vector>

#include "stage1_decode_route.h"

int main() {
  using namespace cldn;
  DevPlan P = {};
  P.point_step = 12;
  P.n_ops = 3;
  P.all_varint = 1u;
  for (uint32_t k = 0; k < 3u; ++k) {
    P.ops[k].kind = OP_QF32;
    P.ops[k].size = 4;
    P.ops[k].offset = 4u * k;
    P.ops[k].max_bytes = 5;
    P.max_regular_bytes += 5u;
    P.min_regular_bytes += 1u;
  }
  for (int call = 0; call < 3; ++call) {
    DecodeFacts F = {};
    F.n_chunks = call == 2 ? 0u : 12u;
    F.wp_parts = 1u;
    F.out_aligned16 = true;
    F.zstd = true;
    F.zstd_seq = call >= 1;
    std::vector<const char*> k;
    decode_route_kernels(decode_route(P, F), k);
    for (const char* n : k) printf("%s ", n);
    printf("\n");
  }
  return 0;
}
