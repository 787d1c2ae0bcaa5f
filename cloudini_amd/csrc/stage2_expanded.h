// stage2_expanded.h -- the two table kernels of cldn_hip_decode_lz4_gather / _zstd_gather (included by stage1_decode.hip).
// A chunk the caller expanded has its stage-1 payload in its slot already (uploaded in front of the launch): its compressed
// bytes are neither decoded nor judged. k_stage2_hold_expanded runs behind the chunk walk and takes such chunks out of the
// stage-2 kernels' sight (they decode entries with valid == 1 only); k_stage2_place_expanded runs behind the stage-2 kernels,
// points the held entries at their slots -- what the decoders leave for a chunk they decompressed -- and writes a verdict
// per chunk. The decoders themselves (lz4_decode.hip, zstd_decode.hip, zstd_seq_decode.hip) are what the contiguous calls run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_device.h"
#include "stage1_launch.h"

namespace cldn {

constexpr uint32_t kDecChunkHeld = 3u;  // DecChunk::valid between the two kernels: an expanded chunk of a sound chunk chain

// zstd_sizes: ZstdDecodeLaunch::sizes of a ZSTD call (k_zstd_walk writes the entries of the frames it walks, nothing else), or NULL
__global__ __launch_bounds__(256) void k_stage2_hold_expanded(DecChunk* __restrict__ chunks, uint32_t n_chunks,
                                                              const uint32_t* __restrict__ expanded_sizes,
                                                              uint32_t* __restrict__ zstd_sizes) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_chunks) return;
  const uint32_t valid = chunks[c].valid;
  const uint32_t size = expanded_sizes[c];
  const bool held = valid == 1u && size != kNotExpanded;
  if (held) chunks[c].valid = kDecChunkHeld;
  if (zstd_sizes && (held || valid != 1u)) zstd_sizes[c] = held ? size : kZdSizeCorrupt;  // (a damaged chain: refused)
}

__global__ __launch_bounds__(256) void k_stage2_place_expanded(DecChunk* __restrict__ chunks, uint32_t n_chunks,
                                                               const uint32_t* __restrict__ expanded_sizes,
                                                               const uint32_t* __restrict__ zstd_sizes, uint64_t slot_stride,
                                                               uint32_t* __restrict__ verdicts) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n_chunks) return;
  const uint32_t valid = chunks[c].valid;
  uint32_t verdict;
  if (valid == kDecChunkHeld) {
    verdict = expanded_sizes[c];
    chunks[c].src_off = (uint64_t)c * slot_stride;
    chunks[c].src_size = verdict;
    chunks[c].valid = 1u;
  } else if (valid == 1u) {
    verdict = chunks[c].src_size;  // (what the decoder left: the bytes in the slot)
  } else {
    verdict = zstd_sizes ? zstd_sizes[c] : kLz4Rejected;
    if (verdict < kZdSizeHost) verdict = kZdSizeCorrupt;  // (cannot happen: a frame with a size keeps valid == 1)
  }
  verdicts[c] = verdict;
}

}  // namespace cldn
