// stage2_decode_plan.h -- who undoes stage 2 of a run of the batch transcoder's decode direction (TranscodeOptions::
// device_stage2_decode). Two pure functions: decodeGpuPhase (host/batch_transcoder.cpp) acts on what they say and on nothing
// else. Host-only: no HIP call, no kernel header -- a plain C++17 compiler builds it (tests/test_stage2_decode_plan.py).
// DESIGN.md §4 has the protocol.
#pragma once

#include <stdint.h>

#include <vector>

#include "cloudini_hip.h"

namespace cldn {

constexpr uint8_t kS2CompNone = 0, kS2CompLz4 = 1, kS2CompZstd = 2;  // Cloudini::CompressionOption's values

struct Stage2Message {
  uint8_t compression;  // kS2Comp*
  uint32_t n_chunks;
};

enum Stage2Call : uint8_t {
  S2_HOST_STAGE1,  // stage 2 on the host pool, then cldn_hip_decode_stage1: the route without the option
  S2_DEVICE_LZ4,   // cldn_hip_decode_lz4_gather
  S2_DEVICE_ZSTD   // cldn_hip_decode_zstd_gather, the sequences switch on
};

struct Stage2Group {  // messages [first, first + count) of the run go through one call
  uint32_t first, count;
  uint32_t first_chunk, n_chunks;  // their chunks among the run's
  uint8_t call;                    // Stage2Call
};

// The first attempt. Neighbours that take the same call share it; a message with another compression between them ends
// the group (the output order is the input order, and a call takes messages that lie side by side).
inline std::vector<Stage2Group> plan_stage2_groups(bool device_stage2, const Stage2Message* msgs, uint32_t n_msgs) {
  std::vector<Stage2Group> groups;
  uint32_t chunk = 0;
  for (uint32_t i = 0; i < n_msgs; ++i) {
    uint8_t call = S2_HOST_STAGE1;
    if (device_stage2 && msgs[i].compression == kS2CompLz4) call = S2_DEVICE_LZ4;
    if (device_stage2 && msgs[i].compression == kS2CompZstd) call = S2_DEVICE_ZSTD;
    if (groups.empty() || groups.back().call != call) groups.push_back({i, 0u, chunk, 0u, call});
    groups.back().count += 1u;
    groups.back().n_chunks += msgs[i].n_chunks;
    chunk += msgs[i].n_chunks;
  }
  return groups;
}

// What follows a device call that returned `rc` with these verdicts (decoded bytes, 0xfffffffe = needs the host, 0xffffffff =
// refused): the chunks the host decompresses for the one second call. Nothing to expand = no second call: `rc` is the outcome
// (CLDN_HIP_OK, or an error no chunk's stage 2 explains, which goes to the caller as it is). A refused chunk is expanded like
// one that needs the host: the host library judges it, and its refusal is the error a run without the option throws.
struct Stage2Retry {
  bool retry = false;
  uint32_t n_expanded = 0;
  std::vector<uint8_t> expanded;  // [n_chunks] 1 = the second call gets this chunk's payload from the host
};
inline Stage2Retry plan_stage2_retry(int rc, const uint32_t* verdicts, uint32_t n_chunks) {
  Stage2Retry R;
  R.expanded.assign(n_chunks, 0);
  if (rc != CLDN_HIP_ERR_UNSUPPORTED && rc != CLDN_HIP_ERR_CORRUPT) return R;
  for (uint32_t c = 0; c < n_chunks; ++c)
    if (verdicts[c] >= 0xfffffffeu) {
      R.expanded[c] = 1;
      R.n_expanded += 1u;
    }
  R.retry = R.n_expanded != 0u;
  return R;
}

// The second call takes payloads of at most a slot (cldn_hip_stage1_bound(plan, 32768) + 60 bytes). The host pool gives its
// library four bytes more, as the route without the option does; a chunk that fills them is no stage-1 payload of this schema,
// and the whole group then takes S2_HOST_STAGE1, whose error is the one to report.
inline bool stage2_retry_fits(const Stage2Retry& R, const uint32_t* host_sizes, uint64_t slot_capacity) {
  for (size_t c = 0; c < R.expanded.size(); ++c)
    if (R.expanded[c] && host_sizes[c] > slot_capacity) return false;
  return true;
}

}  // namespace cldn
