// stage1_launch.h -- host-callable launchers implemented next to the kernels (stage1_kernels.hip, stage1_decode.hip). The two
// stage-1 launchers decide nothing: EncodeLaunch / DecodeLaunch carry the call's buffers, which kernels run is the route's
// (stage1_encode_route.h: the ABI computes it once per call and sizes its buffers from it; stage1_decode_route.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_decode_route.h"
#include "stage1_device.h"
#include "stage1_encode_route.h"
#include "stage1_report.h"
#include "zstd_decode_walk.h"

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

// ---- stage 2 on the device (lz4_kernels.hip, zstd_kernels.hip): what either writer takes from the call and gives back ----
struct Stage2Io {
  hipStream_t stream;
  const uint8_t* stage1;          // framed stage-1 streams (the payload of chunk c starts at chunk_dst[c] + 4)
  uint64_t stage1_capacity;       // bytes of that buffer (ZSTD: a payload that does not lie inside is not read; LZ4 ignores it)
  const uint64_t* chunk_dst;
  const uint32_t* chunk_payload;
  uint32_t n_chunks;
  const uint32_t* cloud_first_chunk;  // [n_clouds + 1]
  uint32_t n_clouds;
  uint32_t* chunk_sizes;          // [n_chunks]: what chunk_sizes reports (LZ4 block / ZSTD frame of the chunk)
  uint64_t* stream_offsets;       // [n_clouds + 1]
  uint8_t* out;                   // the framed streams: [u32 size][block or frame] per chunk, written by the kernels themselves
  uint64_t out_capacity;
  uint32_t* status;
};

// ---- LZ4 block per chunk (lz4_kernels.hip; parameters shared with oracle/lz4_model.c) ----
constexpr uint32_t kLzSubBytes = 8192;    // a wave parses this much of a payload with its own hash table
constexpr uint32_t kLzHashBits = 11;
constexpr uint32_t kLzMaxMatches = 1024;  // per sub-range (the rest of it leaves as literals)
// CLDN_HIP_STAGE2_LZ4_FAST (round 5): sub-ranges of 4 KiB with a 1024-entry table and 512 matches -- 8.2 KB of LDS per wave
// instead of 16.4, twice the resident waves (round 4 measured 1.53 x the speed for 3 % of the ratio: 0.894 -> 0.922)
constexpr uint32_t kLzFastSubBytes = 4096;
constexpr uint32_t kLzFastHashBits = 10;
constexpr uint32_t kLzFastMaxMatches = 512;
struct LzMatch {
  uint32_t pos;  // in the chunk's payload
  uint16_t len;  // 4 .. kLzSubBytes
  uint16_t off;  // 1 .. kLzSubBytes - 1
};
struct Lz4Launch {
  Stage2Io io;
  uint32_t fast;                  // 1 = the CLDN_HIP_STAGE2_LZ4_FAST parameters
  uint64_t max_subs;              // upper bound of the sub-ranges of the batch (payload bound / sub-range bytes + n_chunks)
  LzMatch* matches;               // [max_subs * kLzMaxMatches] (fast: kLzFastMaxMatches), a buffer of its own
  uint64_t* block_dst;            // [n_chunks]: where [u32 size][block] of a chunk begins in io.out, a buffer of its own
  // the workspace, in this order (carve)
  uint32_t* counts;               // [max_subs]: matches of a sub-range
  uint32_t* last_end;             // [max_subs]: where its last match ends (0 = no match)
  uint32_t* anchor_in;            // [max_subs]: where the literals of its first sequence start
  uint32_t* sub_size;             // [max_subs]: bytes of its sequences
  uint32_t* sub_chunk;            // [max_subs]: chunk of a sub-range
  uint32_t* before;               // [max_subs]: sequence bytes of the chunk's earlier sub-ranges
  uint32_t* next_pos;             // [max_subs]: the chunk's next match behind the sub-range
  uint32_t* block_size;           // [n_chunks]: bytes of the chunk's LZ4 block
  uint32_t* sub_first;            // [n_chunks + 1]: compact sub-range numbering
  static size_t workspace_bytes(uint64_t max_subs, uint32_t n_chunks) {
    return (size_t)(7u * max_subs + (uint64_t)n_chunks + ((uint64_t)n_chunks + 1u)) * sizeof(uint32_t);
  }
  void carve(void* ws, uint64_t max_subs_, uint32_t n_chunks) {
    max_subs = max_subs_;
    counts = (uint32_t*)ws;
    last_end = counts + max_subs;
    anchor_in = last_end + max_subs;
    sub_size = anchor_in + max_subs;
    sub_chunk = sub_size + max_subs;
    before = sub_chunk + max_subs;
    next_pos = before + max_subs;
    block_size = next_pos + max_subs;
    sub_first = block_size + n_chunks;
  }
};
int lz4_launch(const Lz4Launch& L);
// the front of it, which the ZSTD writer with matches shares: k_lz4_plan (sub_first[n_chunks + 1]) and k_lz4_match (matches,
// counts, last_end, sub_chunk: [max_subs] each) over the payloads of `io`
int lz4_launch_match(const Stage2Io& io, uint32_t fast, uint64_t max_subs, uint32_t* sub_first, LzMatch* matches, uint32_t* counts,
                     uint32_t* last_end, uint32_t* sub_chunk);

// ---- ZSTD frame of literal-only blocks per chunk (zstd_kernels.hip; restated in tests/zstd_lit_model.py) ----
constexpr uint32_t kZsBlockBytes = 131072;  // a frame's blocks: consecutive pieces of the payload
constexpr uint32_t kZsMinHuf = 64;          // a block below this is Raw
constexpr uint32_t kZsFourStreams = 256;    // one Huffman stream below, four from here on
constexpr uint32_t kZsDescBytes = 128;      // a tree description: its head byte and at most 127 more
constexpr uint32_t kZsRaw = 0, kZsRle = 1, kZsHuf = 2;  // (the block types of the format)
constexpr uint32_t kZsChunkBad = 0u, kZsChunkPlanned = 1u, kZsChunkFits = 2u;  // chunk_state: k_zstd_plan, k_zstd_offsets
struct ZsBlock {
  uint32_t chunk, off, n;   // the block is [off, off + n) of the chunk's payload
  uint32_t kind;
  uint32_t body;            // bytes behind the 3-byte block header
  uint32_t form, hdr_bytes; // literals section header: size format and bytes
  uint32_t desc_bytes;      // tree description
  uint32_t comp;            // tree description + jump table + streams
  uint32_t stream[4];       // bytes of the streams
  uint32_t rle;             // the byte of an RLE block
  uint32_t n_lit;           // literals: n, or what the kept matches of a block with sequences leave
  // a block with sequences (cldn_hip_codec_set_zstd_matches; n_seq != 0): kind is kZsHuf (Compressed) and the fields above describe
  // its literals section where it is Huffman-coded
  uint32_t n_seq;
  uint32_t lit_kind;        // kZsRaw / kZsRle / kZsHuf literals
  uint32_t lit_bytes;       // the literals section, header included
};
// ---- ... with sequences from the LZ4 match search (zstd_seq_kernels.hip; restated in tests/zstd_match_model.py) ----
struct ZsSeqPlan {
  uint32_t n_seq, n_lit;    // kept matches of a block (0: it stays a literal-only block) and the bytes they leave
};
struct ZsSeqInfo {
  uint32_t bytes;           // the block's sequence bit stream
  uint32_t tail_pos;        // bit position of the closing states
  uint32_t tail_bits;       // match-length, offset and literal-length state and the final 1 bit: 18 bits
  uint32_t pad;
};
// Everything per sequence and per literal is indexed by sub-range: block idx of chunk c owns the sub-ranges from
// sub_first[c] + 16 * (idx - blk_first[c]) on, kLzMaxMatches records and kLzSubBytes literals each.
struct ZstdSeqLaunch {
  uint64_t max_subs;              // as Lz4Launch's, with the standard parameters
  LzMatch* matches;               // [max_subs * kLzMaxMatches], a buffer of its own
  // the workspace, in this order (carve); every array starts at a multiple of 64 bytes
  uint8_t* lits;                  // [max_subs * kLzSubBytes]: the literals of the blocks with sequences, compacted
  uint64_t* seq_bits;             // [max_subs * kLzMaxMatches]: bits of a sequence, in stream order (the last sequence first)
  LzMatch* seqs;                  // [max_subs * kLzMaxMatches]: the kept matches, compacted
  uint32_t* seq_pos;              // [max_subs * kLzMaxMatches]: where those bits start in the block's bit stream
  uint32_t* counts;               // [max_subs]  k_lz4_match
  uint32_t* last_end;             // [max_subs]  k_lz4_match
  uint32_t* sub_chunk;            // [max_subs]  k_lz4_match
  uint32_t* seq_first;            // [max_subs]: kept matches of the block's earlier sub-ranges
  uint32_t* lit_first;            // [max_subs]: literals of the block's earlier sub-ranges
  uint32_t* sub_first;            // [n_chunks + 1]
  ZsSeqPlan* plan;                // [max_blocks]
  ZsSeqInfo* info;                // [max_blocks]
  static size_t up64(size_t v) { return (v + 63u) & ~size_t(63); }
  static size_t workspace_bytes(uint64_t max_subs, uint64_t max_blocks, uint32_t n_chunks) {
    const size_t m = (size_t)max_subs;
    return up64(m * kLzSubBytes) + up64(m * kLzMaxMatches * 8u) * 2u + up64(m * kLzMaxMatches * 4u) + up64(m * 4u) * 5u +
           up64(((size_t)n_chunks + 1u) * 4u) + up64((size_t)max_blocks * sizeof(ZsSeqPlan)) + up64((size_t)max_blocks * sizeof(ZsSeqInfo));
  }
  void carve(void* ws, uint64_t max_subs_, uint64_t max_blocks, uint32_t n_chunks) {
    const size_t m = (size_t)max_subs_;
    uint8_t* p = (uint8_t*)ws;
    auto take = [&p](size_t bytes) {
      uint8_t* at = p;
      p += up64(bytes);
      return at;
    };
    max_subs = max_subs_;
    lits = take(m * kLzSubBytes);
    seq_bits = (uint64_t*)take(m * kLzMaxMatches * 8u);
    seqs = (LzMatch*)take(m * kLzMaxMatches * 8u);
    seq_pos = (uint32_t*)take(m * kLzMaxMatches * 4u);
    counts = (uint32_t*)take(m * 4u);
    last_end = (uint32_t*)take(m * 4u);
    sub_chunk = (uint32_t*)take(m * 4u);
    seq_first = (uint32_t*)take(m * 4u);
    lit_first = (uint32_t*)take(m * 4u);
    sub_first = (uint32_t*)take(((size_t)n_chunks + 1u) * 4u);
    plan = (ZsSeqPlan*)take((size_t)max_blocks * sizeof(ZsSeqPlan));
    info = (ZsSeqInfo*)take((size_t)max_blocks * sizeof(ZsSeqInfo));
  }
};
struct ZstdLaunch {
  Stage2Io io;
  uint64_t max_blocks;            // upper bound of the blocks of the batch (payload bound / block bytes + n_chunks)
  // the workspace, in this order (carve); codes and block_dst start at multiples of 64 bytes
  ZsBlock* blocks;                // [max_blocks]
  uint32_t* codes;                // [max_blocks * 256]: length << 16 | code value
  uint8_t* descs;                 // [max_blocks * kZsDescBytes]
  uint64_t* block_dst;            // [max_blocks + 1]: where a block's header goes in io.out (a chunk's first: its [u32] prefix)
  uint32_t* blk_first;            // [n_chunks + 1]: compact block numbering
  uint32_t* chunk_state;          // [n_chunks]
  const ZstdSeqLaunch* seq = nullptr;  // cldn_hip_codec_set_zstd_matches: blocks may hold sequences; NULL = literal-only blocks
  struct Layout {
    size_t codes, descs, block_dst, blk_first, chunk_state, bytes;
  };
  static Layout layout(uint64_t max_blocks, uint32_t n_chunks) {
    Layout o;
    o.codes = ((size_t)max_blocks * sizeof(ZsBlock) + 63u) & ~size_t(63);
    o.descs = o.codes + (size_t)max_blocks * 256u * sizeof(uint32_t);
    o.block_dst = (o.descs + (size_t)max_blocks * kZsDescBytes + 63u) & ~size_t(63);
    o.blk_first = o.block_dst + (size_t)(max_blocks + 1u) * sizeof(uint64_t);
    o.chunk_state = o.blk_first + (size_t)(n_chunks + 1u) * sizeof(uint32_t);
    o.bytes = o.chunk_state + (size_t)n_chunks * sizeof(uint32_t);
    return o;
  }
  static size_t workspace_bytes(uint64_t max_blocks, uint32_t n_chunks) { return layout(max_blocks, n_chunks).bytes; }
  void carve(void* ws, uint64_t max_blocks_, uint32_t n_chunks) {
    const Layout o = layout(max_blocks_, n_chunks);
    uint8_t* p = (uint8_t*)ws;
    max_blocks = max_blocks_;
    blocks = (ZsBlock*)p;
    codes = (uint32_t*)(p + o.codes);
    descs = p + o.descs;
    block_dst = (uint64_t*)(p + o.block_dst);
    blk_first = (uint32_t*)(p + o.blk_first);
    chunk_state = (uint32_t*)(p + o.chunk_state);
  }
};
int zstd_launch(const ZstdLaunch& L);
// zstd_seq_kernels.hip, called by zstd_launch where L.seq is set: behind k_zstd_plan (match search, per-block plan, compaction,
// sequence coder) and behind k_zstd_emit_lits (the bit streams)
int zstd_seq_launch_front(const ZstdLaunch& L, uint32_t max_blocks);
int zstd_seq_launch_emit(const ZstdLaunch& L, uint32_t max_blocks);

// ---- LZ4 blocks back into bytes on the device (lz4_decode.hip) ----
constexpr uint32_t kLz4Rejected = 0xffffffffu;  // sizes[k] of a block the strict rules refuse
struct Lz4DecompressLaunch {
  hipStream_t stream;
  const uint8_t* blocks;          // device; block k = [block_offsets[k], block_offsets[k + 1])
  const uint64_t* block_offsets;  // device [n_blocks + 1]
  uint32_t n_blocks;
  uint8_t* out;                   // device; block k may write [out_offsets[k], out_offsets[k + 1])
  const uint64_t* out_offsets;    // device [n_blocks + 1]
  uint32_t* sizes;                // device [n_blocks]: decoded bytes, or kLz4Rejected
  uint32_t* status;               // ST_CORRUPT when a block is refused
};
int lz4_configure_decode();
int lz4_launch_decompress(const Lz4DecompressLaunch& L);
// the chunks of a decode call: chunk c (valid, src_off / src_size = its block in `streams`) -> slot c; on success the entry
// points at the slot (src_off = c * slot_stride, src_size = decoded bytes), a refused block clears `valid` and raises ST_CORRUPT
int lz4_launch_decode_chunks(hipStream_t stream, const uint8_t* streams, DecChunk* chunks, uint32_t n_chunks, uint8_t* slots,
                             uint64_t slot_stride, uint32_t capacity, uint32_t* status);

// ---- ZSTD frames without sequences back into bytes on the device (zstd_decode.hip, zstd_decode_walk.h) ----
struct ZstdDecodeLaunch {
  hipStream_t stream;
  const uint8_t* frames;          // device
  uint32_t n_frames;
  uint8_t* out;                   // device
  uint32_t* sizes;                // device [n_frames], 4-byte aligned: decoded bytes, kZdSizeCorrupt or kZdSizeHost
  uint32_t* status;               // ST_CORRUPT | ST_ZSTD_REJECT when a frame is refused, ST_ZSTD_HOST when one needs the host
  // either: frame k = [frame_offsets[k], frame_offsets[k + 1]) of `frames`, it may write [out_offsets[k], out_offsets[k + 1]) of `out`
  const uint64_t* frame_offsets;  // device [n_frames + 1]
  const uint64_t* out_offsets;    // device [n_frames + 1]
  // or (chunks != NULL) the chunks of a decode call: chunk c (valid == 1, src_off / src_size = its frame in `frames`) -> slot c of
  // `out`; on success the entry points at the slot, any other verdict clears `valid`
  DecChunk* chunks;
  uint64_t slot_stride;
  uint32_t capacity;
  // the workspace (carve); recs and weights start at multiples of 256 bytes
  uint32_t max_recs;              // block records of the batch (records_for)
  ZdBlock* recs;                  // [max_recs]
  uint8_t* weights;               // [max_recs * 256]: the weights of record i's tree description
  ZdFse* fse;                     // [1024]: scratch of the walk's lanes
  uint64_t* frame_src;            // [n_frames]: where a frame starts in `frames`
  uint64_t* frame_dst;            // [n_frames]: where its content starts in `out`
  uint32_t* n_recs;               // records in use
  // frames with sequences (cldn_hip_codec_set_zstd_sequences; zstd_seq_decode.hip). seq == 0: none of this exists, and a frame
  // with sequences is HOST. The scratch is sized from the bytes `out` may take (seq_out_bytes): a frame's literals lie at its
  // content's offset in `lit`, its sequences from slot (offset + 2) / 3 of `seqbuf`
  uint32_t seq;
  ZdSeqBlock* srecs;              // [max_recs]: next to recs
  ZdSeqSums* frame_sums;          // [n_frames]
  uint32_t* frame_first;          // [n_frames]: the frame's first record
  uint32_t* frame_nrec;           // [n_frames]: its records if it is one the execution takes, else 0
  uint64_t* seqbuf;               // [seq_out_bytes / 3 + 1]: ll | (ml - 3) << 17 | offset value << 34
  uint8_t* lit;                   // [seq_out_bytes]
  // the sum of zd_record_limit over the frames is at most this (out_bytes: the sum of the frames' capacities)
  // (seq: of zd_record_limit_seq)
  static uint32_t records_for(uint32_t n_frames, uint64_t src_bytes, uint64_t out_bytes, bool seq = false) {
    const uint64_t n = (seq ? 4u : 2u) * (uint64_t)n_frames + src_bytes / (seq ? 16u : 256u) + out_bytes / kZdBlockMax;
    return n > 0x7fffff00ull ? 0x7fffff00u : (uint32_t)n;
  }
  static size_t seq_bytes(uint32_t max_recs, uint32_t n_frames, uint64_t seq_out_bytes) {
    return (size_t)max_recs * sizeof(ZdSeqBlock) + (size_t)n_frames * (sizeof(ZdSeqSums) + 8u) + ((size_t)(seq_out_bytes / 3u) + 1u) * 8u +
           (size_t)seq_out_bytes + 1024u;
  }
  // seq_on: the sequences switch; seq_out_bytes: the bytes of `out` the frames may write (0 is a size like any other)
  static size_t workspace_bytes(uint32_t max_recs, uint32_t n_frames, bool seq_on = false, uint64_t seq_out_bytes = 0u) {
    return (((size_t)max_recs * sizeof(ZdBlock) + 255u) & ~size_t(255)) + (size_t)max_recs * 256u + 1024u * sizeof(ZdFse) +
           (size_t)n_frames * 16u + 256u + (seq_on ? seq_bytes(max_recs, n_frames, seq_out_bytes) : 0u);
  }
  void carve(void* ws, uint32_t max_recs_, uint32_t n_frames_, bool seq_on = false, uint64_t seq_out_bytes = 0u) {
    uint8_t* p = (uint8_t*)ws;
    max_recs = max_recs_;
    recs = (ZdBlock*)p;
    p += ((size_t)max_recs * sizeof(ZdBlock) + 255u) & ~size_t(255);
    weights = p;
    p += (size_t)max_recs * 256u;
    fse = (ZdFse*)p;
    p += 1024u * sizeof(ZdFse);
    frame_src = (uint64_t*)p;
    frame_dst = frame_src + n_frames_;
    n_recs = (uint32_t*)(frame_dst + n_frames_);
    seq = seq_on ? 1u : 0u;
    if (!seq) return;
    auto up = [](uint8_t* q) { return (uint8_t*)(((uintptr_t)q + 255u) & ~(uintptr_t)255u); };
    p = up((uint8_t*)(n_recs + 1));
    srecs = (ZdSeqBlock*)p;
    p += (size_t)max_recs * sizeof(ZdSeqBlock);
    frame_sums = (ZdSeqSums*)p;
    p += (size_t)n_frames_ * sizeof(ZdSeqSums);
    frame_first = (uint32_t*)p;
    frame_nrec = frame_first + n_frames_;
    p = up((uint8_t*)(frame_nrec + n_frames_));
    seqbuf = (uint64_t*)p;
    p += ((size_t)(seq_out_bytes / 3u) + 1u) * 8u;
    lit = up(p);
  }
};
static_assert(sizeof(ZdFse) % 8 == 0 && sizeof(ZdBlock) == 48 && sizeof(ZdSeqBlock) == 48 && sizeof(ZdSeqSums) == 40, "workspace layout");
int zstd_launch_decode(const ZstdDecodeLaunch& L);  // the walk + the block decoder (+ zstd_launch_seq with L.seq)
int zstd_launch_seq(const ZstdDecodeLaunch& L);     // zstd_seq_decode.hip: the sequence decoder + the execution
// Bytes of k_zstd_seq_exec's LDS ring (dynamic LDS of the launch): a match further back reads global memory. 32 KiB, not the
// 64 KiB of lz4_decode.hip's: a workgroup is one wave, and with 64 KiB only two of them fit a CU's 160 KiB. Measured on 992
// frames (32 x 1 M XYZI, profiles/r20_a_zstd_seq_trace.txt's call): the kernel took 8.1 ms with 64 KiB against 4.5 ms with 32.
constexpr uint32_t kZdSeqRing = 32768u;
uint32_t zstd_seq_ring_bytes();

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
