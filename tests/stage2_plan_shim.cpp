// C entry points around cloudini_amd/csrc/stage2_decode_plan.h for tests/test_stage2_decode_plan.py (built with g++, no HIP).
#include <stdint.h>
#include <string.h>

#include "stage2_decode_plan.h"

using namespace cldn;

extern "C" {

// msgs: [n][2] = compression, n_chunks. out: [n_groups][5] = first, count, first_chunk, n_chunks, call. Returns the groups.
int plan_groups(int device_stage2, const uint32_t* msgs, uint32_t n, uint32_t* out, uint32_t out_cap) {
  std::vector<Stage2Message> m(n);
  for (uint32_t i = 0; i < n; ++i) m[i] = {(uint8_t)msgs[2 * i], msgs[2 * i + 1]};
  const std::vector<Stage2Group> g = plan_stage2_groups(device_stage2 != 0, m.data(), n);
  if (g.size() > out_cap) return -1;
  for (size_t k = 0; k < g.size(); ++k) {
    const uint32_t row[5] = {g[k].first, g[k].count, g[k].first_chunk, g[k].n_chunks, g[k].call};
    memcpy(out + 5 * k, row, sizeof(row));
  }
  return (int)g.size();
}

// expanded: [n_chunks] out. Returns n_expanded, or -1 when the plan has no second call.
int plan_retry(int rc, const uint32_t* verdicts, uint32_t n_chunks, uint8_t* expanded) {
  const Stage2Retry R = plan_stage2_retry(rc, verdicts, n_chunks);
  if (R.expanded.size() != n_chunks) return -2;
  if (n_chunks) memcpy(expanded, R.expanded.data(), n_chunks);
  if (R.retry != (R.n_expanded != 0u)) return -3;
  return R.retry ? (int)R.n_expanded : -1;
}

int plan_retry_fits(int rc, const uint32_t* verdicts, uint32_t n_chunks, const uint32_t* host_sizes, uint64_t capacity) {
  const Stage2Retry R = plan_stage2_retry(rc, verdicts, n_chunks);
  return stage2_retry_fits(R, host_sizes, capacity) ? 1 : 0;
}

int plan_codes(int which) { return which == 0 ? CLDN_HIP_ERR_UNSUPPORTED : which == 1 ? CLDN_HIP_ERR_CORRUPT : CLDN_HIP_ERR_ARG; }
}
