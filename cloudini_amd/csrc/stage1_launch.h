// stage1_launch.h -- host-callable launchers implemented next to the kernels (stage1_kernels.hip, stage1_decode.hip). The two
// stage-1 launchers decide nothing: EncodeLaunch / DecodeLaunch carry the call's buffers, which kernels run is the route's
// (stage1_encode_route.h: the ABI computes it once per call and sizes its buffers from it; stage1_decode_route.h).
// The launch structs of stage 2 on the device (LZ4 and ZSTD, either direction) are stage2_launch.h, included here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_decode_route.h"
#include "stage1_device.h"
#include "stage1_encode_route.h"
#include "stage1_report.h"
#include "stage2_launch.h"

namespace cldn {

struct EncodeLaunch {
  const DevPlan* plan;
  const EncodeRoute* route;   // encode_route() of the call: the kernels, and the geometry of slots and segment table
  hipStream_t stream;
  const uint8_t* points;      // device, batch AoS
  const uint8_t* points_end;
  const ChunkDesc* chunks;    // device [n_chunks]
  uint32_t n_chunks;
  uint32_t n_clouds;
  const uint32_t* cloud_first_chunk;  // device [n_clouds + 1]
  uint8_t* slots;             // device [n_chunks * route->slot_stride]
  Seg* segs;                  // device [n_chunks * route->segs_per_chunk]
  ColumnPtrs cols;
  PreTokenPtrs pre;           // Gorilla token buffers (read side, by value into the kernels)
  uint4* const* pre_out;      // device array [n_gorilla] of the same buffers (write side of k_gorilla_tokens)
  uint16_t* ranks[kMaxAdaptive];
  uint32_t* chunk_payload;    // device [n_chunks]
  uint64_t* chunk_dst;        // device [n_chunks]
  uint64_t* stream_offsets;   // device [n_clouds + 1]
  uint8_t* modes;             // device [n_clouds * n_adaptive]
  uint8_t* fallback_flags;    // device [n_chunks * n_adaptive], zeroed per call: 1 = section written by a fast path
  // chunk-table output (no framing): the call ends with the chunks' payloads in their slots (segment table) and k_chunk_sizes
  uint32_t* contiguous_flag;       // device word, 0 at launch: set to 1 when a chunk's payload is not one run of its slot
  // k_finish (stage1_finish.h)
  unsigned long long* fin_rec;     // device [n_chunks]: look-back records, tagged with fin_epoch
  unsigned long long* fin_rec2;    // device [n_chunks]
  unsigned long long* fin_anchor;  // device [n_chunks / 1024 + 1], zero at launch
  uint32_t fin_epoch;              // != 0, changes with every call
  uint32_t* fin_ticket;            // device, zero at launch
  uint32_t use_ticket;             // k_finish takes its workgroups' order from the ticket counter (retry after ST_FINISH_TIMEOUT)
  uint32_t test_timeout;           // test hook: see FinishArgs
  uint8_t* out;               // device, framed streams
  uint64_t out_capacity;
  uint32_t* status;           // device status word
  hipEvent_t* events;         // 5 events (start, before regular, after regular, after sections, end) or NULL
  // piece kernel (stage1_fused.h): one wave per piece, every workgroup leaves one segment in the chunk's slot
  const PieceDesc* pieces;    // device [n_pieces] (ER_PIECES)
  uint32_t n_pieces;          // multiple of 4
  unsigned long long* wgrec;  // device [n_chunks * 32]: the workgroups' look-back records (intra), tagged with fin_epoch
  // the caller's device array [n_clouds * n_adaptive] or NULL: where route->writes_caller_modes, the piece kernel's probe
  // workgroups store every mode there as well as to `modes` (else the caller copies `modes`)
  uint8_t* caller_modes;
  // WIDE route (stage1_wide.h): schemas beyond the launch-argument plan; `plan` holds only the scalar members
  const WidePlan* wide;       // host copy of the descriptor (its arrays are device memory), or NULL
  const DevOp* wide_ops_host; // host copy of the regular ops (the Gorilla pre-pass is launched per group of them)
  uint8_t* wide_scratch;      // device [n_chunks * stage1_wide_scratch_bytes()]
  const uint4* const* wide_pre;  // device [n_gorilla] token buffers (same array as pre_out)
};
size_t stage1_wide_scratch_bytes();  // per chunk

struct DecodeLaunch {
  const DevPlan* plan;
  hipStream_t stream;
  uint32_t uses_v5;
  const uint8_t* streams;             // device: framed stage-1 streams of the batch
  const uint64_t* stream_offsets;     // device [n_clouds + 1]
  const uint64_t* cloud_first_point;  // device [n_clouds + 1]
  const uint32_t* cloud_first_chunk;  // device [n_clouds + 1]
  const uint64_t* h_stream_offsets;   // host copies of the three tables: calls of a few clouds pass them as a kernel argument
  const uint64_t* h_cloud_first_point;  // (then the device pointers above may be NULL)
  const uint32_t* h_cloud_first_chunk;
  uint32_t n_clouds;
  uint32_t n_chunks;
  uint32_t dv_hint;                   // what the codec's earlier calls saw: 1 = no chunk had a lone DeltaVarint section, 2 = every chunk had, 0 = unknown / mixed
  DecChunk* chunks;                   // device [n_chunks]: the table k_build_chunks / k_walk_chunks fill
  uint32_t* reg_end;                  // device [n_chunks]: end of the regular stream per chunk (fast path)
  uint8_t* sec_done;                  // device [n_chunks]: 1 = the chunk's sections are decoded (k_decode_general skips them)
  uint8_t* cols[8];                   // device: dense columns of the first adaptive fields (n_points * bpv each), or NULL
  uint32_t* reg_end_pre;              // device [n_chunks]: where k_locate_sections found the regular stream's end (read by the column kernels and the decoder behind them)
  uint8_t* sec_cols;                  // device [n_chunks]: 1 = the columns hold the chunk's integer fields
  const uint32_t* chunk_sizes;        // device [n_chunks] or NULL: the payload sizes, if the caller knows them (no serial walk)
  uint32_t* token_ends;           // the marker kernels' bitmap (k_mark_token_ends, k_mark_ends_automaton): one bit per stream byte (+ a word per chunk), or NULL
  uint32_t fill_zero;             // CLDN_HIP_FILL_ZERO: bytes of a point that no field covers may be written as 0
  uint32_t* slices_done;          // [n_chunks] DeltaVarint slices of a chunk that k_sections_cols_fast finished
  unsigned long long* slice_rec;  // [n_chunks * 48 * 2] (count, sum) records of the slices, tagged with slice_epoch
  uint32_t slice_epoch;           // != 0, different from every earlier launch on slice_rec since it was cleared
  DecChunk* dsec;                 // [n_adaptive * n_chunks]: the sections k_section_offsets sized (stage1_decode_sections_w.h), or NULL
  uint8_t* secs_ok;               // [n_chunks]
  uint32_t* done_cnt;             // [n_chunks]
  uint8_t* out;                       // device: decoded AoS points
  uint32_t* status;
  uint32_t palette_hint;              // the codec's last decode call folded every chunk's section as a small Palette found by
                                      // the point kernel's own guess: the kernels that locate sections and decode them into columns
                                      // are not launched (a chunk that is different after all goes to k_decode_tail's section decoders)
  hipEvent_t* events;                 // 4 events (start, before / behind the regular-stream kernel, end) or NULL
  // WIDE route: the serial decoder with the plan in device memory (schemas beyond the launch-argument plan)
  const WidePlan* wide;               // host copy of the descriptor, or NULL
  void* wide_state;                   // device [n_chunks * n_ops * 16]: the decoder's per-op state
  // SPLIT launches of the point kernel (small batches; stage1_decode_wave.h): NULL = never split
  void* wp_split;                     // device [wp_split_bytes(n_chunks, wp_maxp)]
  uint32_t wp_maxp;                   // pieces (992 bytes) a chunk's payload may have
  uint32_t wp_parts;                  // workgroups per chunk of the point decoder's launch (1 = chained; wp_split_parts or the test hook)
  // cldn_hip_decode_lz4: `streams` holds [u32 block size][LZ4 block] per chunk. Behind the walk, lz4_launch_decode_chunks
  // (lz4_decode.hip) decompresses chunk c into lz4_slots + c * lz4_slot_stride and points the chunk table there: every
  // kernel behind it reads the slots as its stream buffer. NULL = the streams are stage-1 streams.
  uint8_t* lz4_slots;                 // device [n_chunks * lz4_slot_stride]
  uint64_t lz4_slot_stride;           // multiple of 16, >= lz4_capacity
  uint32_t lz4_capacity;              // what a block may decode to (what the host path gives LZ4_decompress_safe)
  // cldn_hip_decode_zstd: the same slots (lz4_slots, lz4_slot_stride, lz4_capacity) filled from [u32 size][ZSTD frame] chunks
  // by zstd_launch_decode (zstd_decode.hip) with this workspace; NULL = not a ZSTD call
  const struct ZstdDecodeLaunch* zstd;
  // cldn_hip_decode_lz4_gather / _zstd_gather (stage2_expanded.h): chunks whose stage-1 payload the caller has put into their
  // slots are kept from the stage-2 kernels and enter the table behind them; every chunk gets a verdict. NULL = neither.
  const uint32_t* expanded_sizes;     // device [n_chunks]: payload bytes in the slot, or kNotExpanded
  uint32_t* verdicts;                 // device [n_chunks]: decoded bytes, kZdSizeHost or kZdSizeCorrupt (= kLz4Rejected)
};
constexpr uint32_t kNotExpanded = 0xffffffffu;
// bytes of the SPLIT workspace: per piece t0 (4) + aggregates (5 x 4) + carries (4 x 4), per chunk 4 flag words
inline size_t wp_split_bytes(uint32_t n_chunks, uint32_t maxp) { return (size_t)n_chunks * maxp * 40u + (size_t)n_chunks * 16u + 256u; }
// Launch errors go to the ABI's thread-local error string (cldn_hip_last_error), implemented in hip_abi.hip.
int launch_fail(hipError_t e, const char* what);

// one launch, checked: the error text names the kernel
template <class Kernel, class... Args>
int launch(const char* name, Kernel kernel, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream, const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : launch_fail(e, name);
}
#define TRY_LAUNCH(...)                                      \
  do {                                                       \
    if (const int rc_ = launch(__VA_ARGS__)) return rc_;     \
  } while (0)

// A launch with more than the 64 KiB of dynamic LDS a runtime grants by default needs hipFuncAttributeMaxDynamicSharedMemorySize:
// stage1_configure_kernels / _decode pass their kernels through here with the most dynamic LDS a launch of each takes.
template <class Kernel>
inline hipError_t allow_lds(Kernel* kernel, uint32_t lds) {
  if (lds <= 65536u) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

int stage1_configure_kernels();
int stage1_configure_decode();   // decode TU (stage1_decode.hip); called by stage1_configure_kernels
int stage1_launch_encode(const EncodeLaunch& L);
int stage1_launch_decode(const DecodeLaunch& L);
int stage1_launch_decode_unframed(const DevPlan& plan, hipStream_t stream, const uint8_t* payload, uint32_t size,
                                  uint32_t capacity_points, void* chunk_slot, uint8_t* out, uint32_t* status,
                                  const WidePlan* wide = nullptr, void* wide_state = nullptr);

// k_finish alone (no section work): frames the chunks of a batch -- one or more segments per chunk in per-chunk slots --
// as [u32 size][bytes] streams. Used for the chunks the device-side stage 2 leaves (lz4_kernels.hip).
struct FrameLaunch {
  hipStream_t stream;
  const ChunkDesc* chunks;
  uint32_t n_chunks;
  const uint32_t* cloud_first_chunk;
  uint32_t n_clouds;
  const uint8_t* slots;
  uint64_t slot_stride;
  const Seg* segs;
  uint32_t segs_per_chunk;
  unsigned long long* rec;     // [n_chunks], tagged with epoch
  unsigned long long* anchor;  // [n_chunks / 1024 + 1], zero at launch
  uint32_t epoch;
  uint32_t* ticket;            // zero at launch
  uint32_t use_ticket;
  uint32_t test_timeout;
  uint32_t* chunk_payload;     // out
  uint64_t* chunk_dst;         // out
  uint64_t* stream_offsets;    // out
  uint8_t* out;
  uint64_t out_capacity;
  uint32_t* status;
};
int stage1_launch_frame(const FrameLaunch& F);

// applyVizLossyPreprocessing for a ragged batch of clouds (viz_kernels.hip)
constexpr uint32_t kVizBlockPoints = 1024;  // points per workgroup; blocks are cut per cloud, a cloud's last one may be partial
struct VizCloud {                 // per cloud, built on the host with the batch shape
  uint64_t first_point;           // of the cloud in the batch
  uint64_t n_points;              // < 2^32 - 1
  uint64_t tab_base;              // first slot of the cloud's table region, counted from the start of its group's tables
  uint64_t cap_mask;              // viz_table_capacity(n_points) - 1
  uint32_t first_block;           // the cloud's blocks are [first_block, next cloud's first_block)
  uint32_t reserved;
};
struct VizBlock {
  uint32_t cloud;
  uint32_t first;                 // cloud-local index of the block's first point
};
static_assert(sizeof(VizCloud) == 40 && sizeof(VizBlock) == 8, "tests/workspace_shim.cpp carves the tables with stand-ins of these sizes");
struct VizGroup {                 // consecutive clouds whose tables share the table memory
  uint32_t first_block, n_blocks;
  uint64_t table_slots;           // sum of the group's table capacities
};
struct VizLaunch {
  hipStream_t stream;
  const uint8_t* points;          // device AoS, clouds back to back
  uint32_t n_clouds;
  uint32_t n_blocks;              // of the whole batch
  uint32_t point_step;
  uint32_t xyz_offset;
  float inv_res;
  const VizCloud* clouds;         // device [n_clouds]
  const VizBlock* blocks;         // device [n_blocks]
  const VizGroup* groups;         // HOST [n_groups]
  uint32_t n_groups;
  unsigned long long* keys;       // device: {key, first index, pad} per slot, room for the largest group
  uint32_t* slot_of;              // device [points of the batch]
  unsigned long long* keep_bits;  // device [16 n_blocks]: one bit per point
  uint32_t* block_count;          // device [n_blocks]: survivors per block, then the block's output position
  unsigned long long* kept;       // device [n_clouds + 1]: surviving points per cloud, total
  uint8_t* out;                   // device: survivors of all clouds back to back
};
uint64_t viz_table_capacity(uint64_t n_points);
int viz_launch(const VizLaunch& L);

// ---- per-field error report of two point buffers (audit_kernels.hip; record: cldn_hip_audit_field_t, five 64-bit words) ----
// Clouds, blocks, the staged route and the field table as a kernel argument are stage1_report.h's, for all three report kernels.
constexpr uint32_t kAuditLdsBytes = 65536 - 256;  // dynamic LDS of the staged route: both buffers' stage, next to the reduction records
struct AuditField {
  uint32_t offset;
  uint8_t size;      // 1, 2, 4, 8
  uint8_t is_float;  // FLOAT32 / FLOAT64: compared as numbers as well as bytes
  uint8_t pad[2];
  double limit;      // >= 0
};
static_assert(sizeof(AuditField) == 16, "128 of them are a kernel argument");
struct AuditLaunch {
  hipStream_t stream;
  const uint8_t* a;              // device AoS, clouds back to back, any alignment
  const uint8_t* b;
  uint32_t point_step;
  uint32_t n_clouds;
  uint32_t n_blocks;
  uint32_t n_fields;
  const AuditField* fields;      // HOST [n_fields]
  const AuditField* dev_fields;  // device copy of it, or NULL when n_fields <= kReportArgFields
  const ReportCloud* clouds;     // device [n_clouds]
  const ReportBlock* blocks;     // device [n_blocks]
  unsigned long long* report;    // device [n_clouds * n_fields * 5], 8-byte aligned: cleared, then filled
};
int audit_launch(const AuditLaunch& L);            // one clear + one kernel

// ---- resolution sweep of the lossy float fields (sweep_kernels.hip; record: cldn_hip_sweep_cell_t, four 64-bit words) ----
// kReportBlockPoints = 1024 divides 32768: a block never straddles a chunk.
constexpr uint32_t kSweepMaxCandidates = 16;      // CLDN_HIP_SWEEP_MAX_CANDIDATES
constexpr uint32_t kSweepLdsBytes = 40960;        // dynamic LDS of the staged route: one predecessor point + the stage's points
enum SweepKind : uint8_t { SWEEP_NONE = 0, SWEEP_QF32 = 1, SWEEP_F32 = 2, SWEEP_F64 = 3 };  // the field's encoder: OP_QF32 / OP_LOSSY_F32 / OP_LOSSY_F64
struct SweepField {
  uint32_t offset;
  uint8_t kind;      // SweepKind
  uint8_t pad[3];
};
static_assert(sizeof(SweepField) == 8, "128 of them are a kernel argument");
struct SweepCand {   // one rung of a field's ladder; m == 0: skip
  double m;          // the encoder's multiplier (a float32 value for the FLOAT32 kinds: exact in a double)
  double r;          // (double)resolution: the decoder's factor (a float32 value for the FLOAT32 kinds) and the limit
};
struct SweepLaunch {
  hipStream_t stream;
  const uint8_t* points;         // device AoS, clouds back to back, any alignment
  uint32_t point_step;
  uint32_t n_clouds;
  uint32_t n_blocks;
  uint32_t n_fields;
  uint32_t n_candidates;         // 1..kSweepMaxCandidates
  const SweepField* fields;      // HOST [n_fields]
  const SweepField* dev_fields;  // device copy of it, or NULL when n_fields <= kReportArgFields
  const SweepCand* cands;        // device [n_fields * n_candidates]
  const ReportCloud* clouds;     // device [n_clouds]
  const ReportBlock* blocks;     // device [n_blocks]
  unsigned long long* report;    // device [n_clouds * n_fields * n_candidates * 4], 8-byte aligned: cleared, then filled
};
int sweep_launch(const SweepLaunch& L);            // one clear + one kernel

// ---- byte histograms for the stage-2 estimate (hist_kernels.hip; record: cldn_hip_hist_t, 256 64-bit words) ----
// k_sweep_hist takes a SweepLaunch whose report holds [n_clouds * n_fields * n_candidates * 256] words. A workgroup walks
// `walk` consecutive entries of the block table and flushes once per (cloud, field, candidate); 0 = kHistWalkBlocks.
constexpr uint32_t kHistWalkBlocks = 4;           // measured: DESIGN.md 4f (1 .. 32 tried; 2 .. 8 within 4 %, 4 the best of both sets)
constexpr uint32_t kStreamHistItemBytes = 131072; // bytes of a stream per workgroup of k_stream_hist (32 KiB: clearing and summing the 32 copies was a third of the LDS work)
struct StreamHistItem {
  uint64_t begin, end;           // bytes of `streams`
  uint32_t cloud;
  uint32_t pad;
};
struct StreamHistLaunch {
  hipStream_t stream;
  const uint8_t* streams;        // device, any alignment
  uint32_t n_clouds;
  uint32_t n_items;
  const StreamHistItem* items;   // device [n_items]: no item is empty
  unsigned long long* report;    // device [n_clouds * 256], 8-byte aligned: cleared, then filled
};
int sweep_hist_launch(const SweepLaunch& L, uint32_t walk);  // one clear + one kernel
int stream_hist_launch(const StreamHistLaunch& L);           // one clear + one kernel

// ---- CRC-32 of byte spans (crc_kernels.hip; the arithmetic: crc32_combine.h) ----
// A span is cut at absolute addresses: its frame starts at the span's first byte rounded down to kCrcLaneBytes, lane t of
// workgroup j takes the bytes of the span in [frame + j * kCrcSegmentBytes + t * kCrcLaneBytes, ... + kCrcLaneBytes).
constexpr uint32_t kCrcThreads = 256;
constexpr uint32_t kCrcLaneBytes = 128;                                 // one cache line per lane
constexpr uint32_t kCrcWaveBytes = 64u * kCrcLaneBytes;
constexpr uint32_t kCrcSegmentBytes = kCrcThreads * kCrcLaneBytes;      // per workgroup: 32 KiB
struct CrcItem {
  uint64_t begin, end;           // bytes of `streams`, begin < end, inside one segment of the span's frame
  uint32_t span;
  uint32_t mult;                 // x^(8 * bytes of the span behind `end`) mod P
  uint32_t first;                // 1: the span starts here (initial value and final xor go in with this item)
  uint32_t pad;
};
static_assert(sizeof(CrcItem) == 32, "two per 64-byte line");
struct CrcLaunch {
  hipStream_t stream;
  const uint8_t* streams;        // device, any alignment
  uint32_t n_spans;
  uint32_t n_items;
  const CrcItem* items;          // device [n_items]
  uint32_t* crc;                 // device [n_spans], 4-byte aligned: cleared, then filled
};
int stream_crc32_launch(const CrcLaunch& L);                 // one clear + one kernel

// ---- sweep of the V5 adaptive integer modes (mode_kernels.hip; record: cldn_hip_mode_cell_t, five 64-bit words) ----
constexpr uint32_t kModeProbeUnit = 0xffffffffu;  // ModeUnit::chunk of the unit that probes a cloud's first kProbePoints values
struct ModeField {
  uint32_t offset;
  uint8_t type;      // Cloudini::FieldType of the adaptive field
  uint8_t bpv;       // 2, 4, 8
  uint8_t pad[2];
};
static_assert(sizeof(ModeField) == 8, "128 of them are a kernel argument");
struct ModeUnit {    // one workgroup: one section of one adaptive field
  uint32_t cloud;
  uint32_t chunk;    // of the cloud, or kModeProbeUnit
  uint32_t field;    // index among the plan's adaptive fields
  uint32_t pad;
};
struct ModeLaunch {
  hipStream_t stream;
  const uint8_t* points;         // device AoS, clouds back to back, any alignment
  uint32_t point_step;
  uint32_t n_clouds;
  uint32_t n_units;
  uint32_t n_fields;             // adaptive fields of the plan
  const ModeField* fields;       // HOST [n_fields]
  const ModeField* dev_fields;   // device copy of it, or NULL when n_fields <= kReportArgFields
  const ReportCloud* clouds;     // device [n_clouds]
  const ModeUnit* units;         // device [n_units]
  unsigned long long* report;    // device [n_clouds * n_fields * 5], 8-byte aligned: cleared, then filled
};
int modes_configure();
int modes_launch(const ModeLaunch& L);             // one clear + one kernel

}  // namespace cldn
