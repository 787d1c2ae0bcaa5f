// Internal glue between the host translation units (not installed).
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "cloudini_hip.h"
#include "cloudini_lib/cloudini.hpp"

namespace Cloudini {
namespace amd_detail {

// cloudini_ros::applyVizLossyPreprocessing in two parts (src/ros_msg_utils.cpp:249-341). The part that does not look at the
// data: the gate (:250-279 -- a FLOAT32 triple in front, consecutive offsets, one positive finite resolution), which yields
// where the triple sits and the voxel size, and the rule behind the filter (:336-340: a FLOAT64 field without a resolution
// gets 1 us). The data path: cldn_hip_viz_preprocess on host buffers through a pooled codec (throws std::runtime_error), or
// encodeStage1BatchViz below for a whole schema run.
bool vizLossyGate(const std::vector<Cloudini::PointField>& fields, uint32_t point_step, uint32_t* xyz_offset, float* resolution);
void vizLossyStampRule(std::vector<Cloudini::PointField>& fields);
uint64_t vizPreprocessOnDevice(const uint8_t* points, size_t n_points, uint32_t point_step, uint32_t xyz_offset,
                               float resolution, uint8_t* out, size_t out_capacity);

// ---- building blocks of the batch transcoder (batch_transcoder.cpp) ----
// One batched stage-1 encode of n clouds that share `info`'s schema, each in its own host buffer: the framed streams
// ([u32 size][payload] per 32768-point chunk) land back to back in `stage1`; stream_offsets has n + 1 entries,
// chunk_sizes one payload size per chunk in batch order. Throws std::runtime_error.
// `grow(bytes)` is called once with the exact size of the batch's streams and returns where they go (page-locked memory
// makes the copy back fast).
// `audit` (optional): behind the encode call the codec audits it on the device (cldn_hip_audit_last_encode: the points it
// staged against the decode of the streams it wrote); limit = NULL or info.fields.size() doubles, report receives
// n_clouds * info.fields.size() records.
struct AuditRequest {
  const double* limit = nullptr;
  std::vector<cldn_hip_audit_field_t> report;
};
// `sweep` (optional): behind the encode call (and behind the audit, if both are asked for) the codec sweeps the points it
// encoded (cldn_hip_sweep_last_encode; behind the viz filter: the survivors); resolutions = info.fields.size() * n_candidates
// float32, one ladder per field (0 = skip), report receives n_clouds * info.fields.size() * n_candidates cells.
// `estimate`: behind the sweep, the byte histograms for the stage-2 estimate (cldn_hip_sweep_hist_last_encode with the same
// ladders, again with the one-rung ladder own_resolutions -- info.fields.size() float32, 0 = skip --, and
// cldn_hip_stream_hist_last_encode): hist as report, own_hist one per cloud and field, stream_hist one per cloud.
struct SweepRequest {
  const float* resolutions = nullptr;
  uint32_t n_candidates = 0;
  std::vector<cldn_hip_sweep_cell_t> report;
  bool estimate = false;
  const float* own_resolutions = nullptr;
  std::vector<cldn_hip_hist_t> hist, own_hist, stream_hist;
};
// `modes` (optional): right behind the encode call the codec sweeps the adaptive integer modes of the points it encoded
// (cldn_hip_sweep_modes_last_encode; behind the viz filter: the survivors): report receives n_clouds * adaptive_fields cells.
// With apply_best, when some cloud's best mode differs from the probed one, the encode call is repeated ONCE from the same host
// buffers with cldn_hip_codec_force_modes_per_cloud(best modes) and the forcing is cleared again (reencoded = true): the streams
// are then not the reference encoder's bytes, and the audit and the resolution sweep behind it see the second encode.
struct ModesRequest {
  bool apply_best = false;
  uint32_t adaptive_fields = 0;
  std::vector<uint32_t> field_index;  // of each adaptive field among info.fields (cldn_hip_plan_adaptive_field_index)
  bool reencoded = false;
  std::vector<cldn_hip_mode_cell_t> report;
};
// `crc` (optional): behind the encode call (and behind a second one that `modes` made) the CRC-32 and the length of every
// cloud's framed stage-1 stream, taken on the device (cldn_hip_stream_crc32_last_encode): under a device stage 2 the checksum
// of what the blocks or frames decode to.
struct StreamCrcRequest {
  std::vector<uint32_t> crc;
  std::vector<uint64_t> sizes;
};
void encodeStage1Batch(const Cloudini::EncodingInfo& info, const uint8_t* const* cloud_ptrs, const uint64_t* cloud_points,
                       uint32_t n_clouds, const std::function<uint8_t*(uint64_t)>& grow, std::vector<uint64_t>& stream_offsets,
                       std::vector<uint32_t>& chunk_sizes, AuditRequest* audit = nullptr, SweepRequest* sweep = nullptr,
                       ModesRequest* modes = nullptr, int stage2 = 0, StreamCrcRequest* crc = nullptr);
// `stage2` (both calls): the codec's stage-2 mode for the call (cldn_hip_codec_set_stage2; 0 = CLDN_HIP_STAGE2_NONE). With
// CLDN_HIP_STAGE2_ZSTD the streams are [u32 size][ZSTD frame] per chunk and chunk_sizes the frame sizes: finished chunks of
// a ZSTD message, nothing is left for the host's stage 2. kStage2ZstdMatches added to it turns cldn_hip_codec_set_zstd_matches on
// for the call.
constexpr int kStage2ZstdMatches = 0x100;
// The same behind the viz pre-filter (cldn_hip_encode_stage1_viz_gather): every cloud is filtered on its own, the survivors
// are encoded without leaving the device. kept_points gets n_clouds survivor counts; stream_offsets and chunk_sizes describe
// the filtered clouds (a cloud that loses every point has an empty stream and no chunk).
void encodeStage1BatchViz(const Cloudini::EncodingInfo& info, const uint8_t* const* cloud_ptrs, const uint64_t* cloud_points,
                          uint32_t n_clouds, uint32_t xyz_offset, float resolution, const std::function<uint8_t*(uint64_t)>& grow,
                          std::vector<uint64_t>& stream_offsets, std::vector<uint32_t>& chunk_sizes,
                          std::vector<uint64_t>& kept_points, AuditRequest* audit = nullptr, SweepRequest* sweep = nullptr,
                          ModesRequest* modes = nullptr, int stage2 = 0, StreamCrcRequest* crc = nullptr);
// detail::CompressChunk (src/codec_common.cpp:220-258) and its worst-case output size
uint32_t compressChunkTo(Cloudini::CompressionOption opt, const uint8_t* src, size_t src_size, uint8_t* dst, size_t dst_cap);
size_t compressedChunkBound(Cloudini::CompressionOption opt, size_t stage1_bytes);
// ---- the way back (decode direction of the batch transcoder) ----
struct ChunkRef {
  const uint8_t* src;  // stage-2 payload of the chunk (behind its [u32 size])
  uint32_t size;
};
// The chunk chain of one compressed cloud (header already removed), validated like PointcloudDecoder::decode does
// (src/cloudini.cpp:645-664; same error strings). `points` = width * height of the header.
void walkCompressedChunks(Cloudini::ConstBufferView data, uint64_t points, std::vector<ChunkRef>& refs);
// detail::DecompressChunk (src/codec_common.cpp:260-300): LZ4 block / ZSTD frame / plain copy -> stage-1 bytes
// LZ4 streams with stage 2 on the device (cldn_hip_codec_set_stage2): off unless CLOUDINI_AMD_DEVICE_LZ4=1 or the setter
bool deviceLz4();
void setDeviceLz4(bool on);
int deviceLz4Level();            // 0 host pool, 1 CLDN_HIP_STAGE2_LZ4, 2 CLDN_HIP_STAGE2_LZ4_FAST
void setDeviceLz4Level(int level);
// The way back: PointcloudDecoder::decode of an LZ4 message (wire version >= 3) uploads the compressed body and lets
// cldn_hip_decode_lz4 undo stage 2 on the device instead of LZ4_decompress_safe on the host pool. Off by default, no
// environment variable; with it off every path is what it was.
bool deviceZstd();               // PointcloudEncoder::encode with CompressionOption::ZSTD writes the device's literal-only frames
void setDeviceZstd(bool on);     // (default off; valid ZSTD frames, not libzstd's bytes)
// ... with sequences from the device's match search (cldn_hip_codec_set_zstd_matches); it has meaning only while deviceZstd() is
// on; default off, no environment variable
bool deviceZstdMatches();
void setDeviceZstdMatches(bool on);
bool deviceLz4Decode();
void setDeviceLz4Decode(bool on);
// ZSTD messages of frames without sequences through cldn_hip_decode_zstd (PointcloudDecoder::decode); default off
bool deviceZstdDecode();
void setDeviceZstdDecode(bool on);
void countDeviceZstdDecode();
uint64_t deviceZstdDecodeCount();  // messages decoded through cldn_hip_decode_zstd since the library was loaded
// ... and libzstd's own messages too (frames with sequences, cldn_hip_codec_set_zstd_sequences); it has meaning only while
// deviceZstdDecode() is on; default off
bool deviceZstdSequences();
void setDeviceZstdSequences(bool on);

uint32_t decompressChunkTo(Cloudini::CompressionOption opt, const uint8_t* src, size_t size, uint8_t* dst, size_t dst_cap);
// worst-case stage-1 bytes of one 32768-point chunk of this schema (without its [u32 size])
size_t stage1ChunkBound(const Cloudini::EncodingInfo& info);
// One batched stage-1 decode: n clouds of the same schema, framed stage-1 streams back to back in `streams` (offsets has
// n + 1 entries), decoded points back to back in `out` (cloud k: cloud_points[k] * point_step bytes). Bytes of a point that
// no field covers keep the content of `out`, or read 0 with out_is_zero (the caller does not need `out`'s content:
// CLDN_HIP_FILL_ZERO). Throws std::runtime_error.
void decodeStage1Batch(const Cloudini::EncodingInfo& info, const uint8_t* streams, const uint64_t* offsets,
                       const uint64_t* cloud_points, uint32_t n_clouds, uint8_t* out, uint64_t out_capacity,
                       bool out_is_zero = false);
// The same with stage 2 undone on the device (TranscodeOptions::device_stage2_decode): n LZ4 or ZSTD clouds of one schema, body
// k = the chunks of message k behind its Cloudini header, wherever it lies (cldn_hip_decode_lz4_gather / _zstd_gather, the
// sequences switch on for the call). chunk_sizes: what walkCompressedChunks found; expanded / expanded_sizes (or both NULL):
// stage-1 payloads of chunks the caller decompressed; verdicts: [total chunks], written when the device judged the chunks.
// Returns the call's CLDN_HIP_* code and its text in `error`: what to do about CLDN_HIP_ERR_UNSUPPORTED / _CORRUPT is the
// caller's plan (stage2_decode_plan.h). Throws std::runtime_error for what no call was made for.
int decodeStage2Batch(const Cloudini::EncodingInfo& info, const uint8_t* const* bodies, const uint64_t* body_sizes,
                      const uint64_t* cloud_points, uint32_t n_clouds, const uint32_t* chunk_sizes, const uint8_t* const* expanded,
                      const uint32_t* expanded_sizes, uint32_t* verdicts, uint8_t* out, uint64_t out_capacity, bool out_is_zero,
                      std::string& error);
// fn(i) for i in [0, n) on the bounded stage-2 pool (the caller takes part)
void runOnStage2Pool(size_t n, const std::function<void(size_t)>& fn);

// Stage-2 (LZ4/ZSTD) threads per encode()/decode() call, the caller included (bounded worker pool, cloudini.cpp).
unsigned stage2Threads();
void setStage2Threads(unsigned n);

}  // namespace amd_detail
}  // namespace Cloudini
