// stage2_launch.h -- stage 2 on the device: the launch structs of the LZ4 and ZSTD writers (lz4_kernels.hip, zstd_kernels.hip,
// zstd_seq_kernels.hip) and decoders (lz4_decode.hip, zstd_decode.hip, zstd_seq_decode.hip) and their launchers. Each struct
// with a workspace lists its arrays once, in carve() (workspace_carve.h); workspace_bytes() is that carve over NULL. No wave
// intrinsic and no kernel header: a plain C++17 compiler with the HIP headers on its path builds this file
// (tests/test_workspace_carve.py). stage1_launch.h includes it.
#pragma once

#include <hip/hip_runtime.h>

#include "stage1_device.h"
#include "workspace_carve.h"
#include "zstd_decode_walk.h"

namespace cldn {

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
  static size_t workspace_bytes(uint64_t max_subs, uint32_t n_chunks) { return Lz4Launch().carve(nullptr, max_subs, n_chunks); }
  size_t carve(void* base, uint64_t max_subs_, uint32_t n_chunks) {
    Carve ws(base);
    max_subs = max_subs_;
    const size_t m = (size_t)max_subs_;
    counts = ws.take<uint32_t>(m);
    last_end = ws.take<uint32_t>(m);
    anchor_in = ws.take<uint32_t>(m);
    sub_size = ws.take<uint32_t>(m);
    sub_chunk = ws.take<uint32_t>(m);
    before = ws.take<uint32_t>(m);
    next_pos = ws.take<uint32_t>(m);
    block_size = ws.take<uint32_t>(n_chunks);
    sub_first = ws.take<uint32_t>((size_t)n_chunks + 1u);
    return ws.bytes();
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
  static size_t workspace_bytes(uint64_t max_subs, uint64_t max_blocks, uint32_t n_chunks) {
    return ZstdSeqLaunch().carve(nullptr, max_subs, max_blocks, n_chunks);
  }
  size_t carve(void* base, uint64_t max_subs_, uint64_t max_blocks, uint32_t n_chunks) {
    Carve ws(base);
    const size_t m = (size_t)max_subs_;
    max_subs = max_subs_;
    lits = ws.take<uint8_t>(m * kLzSubBytes, 64);
    seq_bits = ws.take<uint64_t>(m * kLzMaxMatches, 64);
    seqs = ws.take<LzMatch>(m * kLzMaxMatches, 64);
    seq_pos = ws.take<uint32_t>(m * kLzMaxMatches, 64);
    counts = ws.take<uint32_t>(m, 64);
    last_end = ws.take<uint32_t>(m, 64);
    sub_chunk = ws.take<uint32_t>(m, 64);
    seq_first = ws.take<uint32_t>(m, 64);
    lit_first = ws.take<uint32_t>(m, 64);
    sub_first = ws.take<uint32_t>((size_t)n_chunks + 1u, 64);
    plan = ws.take<ZsSeqPlan>((size_t)max_blocks, 64);
    info = ws.take<ZsSeqInfo>((size_t)max_blocks, 64);
    ws.take<uint8_t>(0, 64);  // the workspace ends at a multiple of 64 too
    return ws.bytes();
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
  static size_t workspace_bytes(uint64_t max_blocks, uint32_t n_chunks) { return ZstdLaunch().carve(nullptr, max_blocks, n_chunks); }
  size_t carve(void* base, uint64_t max_blocks_, uint32_t n_chunks) {
    Carve ws(base);
    const size_t m = (size_t)max_blocks_;
    max_blocks = max_blocks_;
    blocks = ws.take<ZsBlock>(m);
    codes = ws.take<uint32_t>(m * 256u, 64);
    descs = ws.take<uint8_t>(m * kZsDescBytes);
    block_dst = ws.take<uint64_t>(m + 1u, 64);
    blk_first = ws.take<uint32_t>((size_t)n_chunks + 1u);
    chunk_state = ws.take<uint32_t>(n_chunks);
    return ws.bytes();
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
  // content's offset in `lit`, its sequences from slot (offset + 2) / 3 of `seqbuf`. srecs, seqbuf and lit start at multiples of 256
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
  // seq_on: the sequences switch; seq_out_bytes: the bytes of `out` the frames may write (0 is a size like any other)
  static size_t workspace_bytes(uint32_t max_recs, uint32_t n_frames, bool seq_on = false, uint64_t seq_out_bytes = 0u) {
    return ZstdDecodeLaunch().carve(nullptr, max_recs, n_frames, seq_on, seq_out_bytes);
  }
  size_t carve(void* base, uint32_t max_recs_, uint32_t n_frames_, bool seq_on = false, uint64_t seq_out_bytes = 0u) {
    Carve ws(base);
    max_recs = max_recs_;
    recs = ws.take<ZdBlock>(max_recs, 256);
    weights = ws.take<uint8_t>((size_t)max_recs * 256u, 256);
    fse = ws.take<ZdFse>(1024);
    frame_src = ws.take<uint64_t>(n_frames_);
    frame_dst = ws.take<uint64_t>(n_frames_);
    n_recs = ws.take<uint32_t>(1);
    seq = seq_on ? 1u : 0u;
    if (seq) {
      srecs = ws.take<ZdSeqBlock>(max_recs, 256);
      frame_sums = ws.take<ZdSeqSums>(n_frames_);
      frame_first = ws.take<uint32_t>(n_frames_);
      frame_nrec = ws.take<uint32_t>(n_frames_);
      seqbuf = ws.take<uint64_t>((size_t)(seq_out_bytes / 3u) + 1u, 256);
      lit = ws.take<uint8_t>((size_t)seq_out_bytes, 256);
      ws.pad(1024u);  // slack behind the sequence scratch (no array lies in it)
    }
    ws.pad(256u);  // slack behind the last array, with and without sequences
    return ws.bytes();
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

}  // namespace cldn
