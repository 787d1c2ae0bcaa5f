// cloudini_amd/csrc/stage2_decode_plan.h on the table of tests/test_stage2_decode_plan.py, as a program of its own: built with
// -fsanitize=address,undefined and run on the CPU. Prints one line per case; the test compares them with its own table.
#include <cstdio>
#include <vector>

#include "stage2_decode_plan.h"

using namespace cldn;

static void groups(const char* name, bool on, const std::vector<Stage2Message>& m) {
  std::printf("groups %s", name);
  for (const Stage2Group& g : plan_stage2_groups(on, m.data(), (uint32_t)m.size()))
    std::printf(" %u:%u:%u:%u:%u", g.first, g.count, g.first_chunk, g.n_chunks, (unsigned)g.call);
  std::printf("\n");
}

static void retry(const char* name, int rc, const std::vector<uint32_t>& verdicts) {
  const Stage2Retry R = plan_stage2_retry(rc, verdicts.data(), (uint32_t)verdicts.size());
  std::printf("retry %s %d %u", name, R.retry ? 1 : 0, R.n_expanded);
  for (uint8_t e : R.expanded) std::printf(" %u", (unsigned)e);
  std::printf("\n");
}

int main() {
  const uint8_t N = kS2CompNone, L = kS2CompLz4, Z = kS2CompZstd;
  // three ZSTD messages of 1, 3 and 2 chunks
  const std::vector<Stage2Message> run = {{Z, 1}, {Z, 3}, {Z, 2}};
  groups("zstd_on", true, run);
  groups("zstd_off", false, run);
  groups("none_inside", true, {{L, 2}, {L, 1}, {N, 3}, {L, 1}});
  groups("mixed", true, {{N, 1}, {L, 2}, {Z, 3}, {Z, 0}, {N, 1}});
  groups("empty", true, {});
  retry("all_sizes_ok", CLDN_HIP_OK, {100, 200, 300, 400, 500, 600});
  retry("all_sizes_corrupt", CLDN_HIP_ERR_CORRUPT, {100, 200, 300, 400, 500, 600});  // a malformed stage-1 stream: no second call
  retry("host_middle", CLDN_HIP_ERR_UNSUPPORTED, {100, 200, 0xfffffffeu, 400, 500, 600});
  retry("refused_middle", CLDN_HIP_ERR_CORRUPT, {100, 200, 0xffffffffu, 400, 500, 600});
  retry("both", CLDN_HIP_ERR_CORRUPT, {0xfffffffeu, 200, 0xffffffffu, 400, 500, 0xfffffffeu});
  retry("other_error", CLDN_HIP_ERR_ARG, {0xfffffffeu, 0xffffffffu});
  retry("empty", CLDN_HIP_ERR_CORRUPT, {});
  const std::vector<uint32_t> v = {100, 0xfffffffeu, 300};
  const Stage2Retry R = plan_stage2_retry(CLDN_HIP_ERR_UNSUPPORTED, v.data(), 3);
  const uint32_t fits[3] = {0, 1000, 0}, over[3] = {5000, 1001, 5000};
  std::printf("fits %d %d\n", stage2_retry_fits(R, fits, 1000) ? 1 : 0, stage2_retry_fits(R, over, 1000) ? 1 : 0);
  return 0;
}
